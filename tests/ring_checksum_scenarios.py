"""Expected values of the ring-checksum tests (tests/test_ring_checksum_host.py, tests/test_ring_checksum.py).
TEST INFRASTRUCTURE ONLY.

ringcs(o) = Fingerprint32 of the addresses row o holds alive or suspect, in ascending member index, joined by ';'
(Ringpop.Checksum, ringpop.go:571-577; hashring.go:100-107). Every value comes from the oracle alone: OracleSim.rows()
and live() give the views, oracle_ffi.fingerprint32 hashes the joined string, once per distinct presence set.
"""
import numpy as np

from oracle_ffi import fingerprint32
import swimsim

EMPTY = 3696677242                                # or_fingerprint32("")
MEMBERS_0_TO_4 = 2141723838                       # or_ring_checksum of the synthetic addresses of members 0..4
MODES = (0, 1, 2)


def addresses_of(n, addresses=None):
    return list(addresses) if addresses is not None else [swimsim.address_of(m) for m in range(n)]


def view_checksum(addr, present):
    """the ring checksum of the view that holds the members in the boolean vector `present`"""
    return fingerprint32(";".join(addr[m] for m in np.nonzero(present)[0]).encode())


def expected_rows(status_rows, addresses=None):
    """(checksums uint32 [rows], servers uint32 [rows], distinct views) of status rows [rows, n] (0 alive .. 7 unknown)"""
    status_rows = np.asarray(status_rows)
    addr = addresses_of(status_rows.shape[1], addresses)
    cs = np.empty(len(status_rows), np.uint32)
    srv = np.empty(len(status_rows), np.uint32)
    views = {}                                    # the joined string is hashed once per distinct presence set
    for o, row in enumerate(status_rows):
        present = row <= 1
        key = present.tobytes()
        if key not in views:
            views[key] = view_checksum(addr, present)
        cs[o], srv[o] = views[key], int(present.sum())
    return cs, srv, len(views)


def expected(ora, addresses=None):
    return expected_rows(ora.rows()[0], addresses)


def live_mask(ora, who):
    return np.array([ora.live(o) for o in range(ora.n)], bool) if who == "live" else np.ones(ora.n, bool)


def expected_hist(cs, srv, mask, lo=0):
    """(counted, hist_checksum, hist_count, hist_servers, hist_first) of the rows in mask (row i = observer lo + i)"""
    idx = np.nonzero(mask)[0]
    u, first, cnt = np.unique(cs[idx], return_index=True, return_counts=True)   # first occurrence = lowest observer
    return (len(idx), u.astype(np.uint32), cnt.astype(np.uint32), srv[idx][first].astype(np.uint32),
            (idx[first] + lo).astype(np.uint32))


def distinct_views(status_rows, mask=None):
    rows = np.asarray(status_rows) <= 1
    if mask is not None:
        rows = rows[mask]
    return len({r.tobytes() for r in rows})


def check_hist(got, want, what):
    assert got[0] == want[0], f"{what}: counted {got[0]}, oracle {want[0]}"
    for i, name in enumerate(("hist_checksum", "hist_count", "hist_servers", "hist_first"), start=1):
        assert len(got[i]) == len(want[i]) and (np.asarray(got[i]) == want[i]).all(), \
            f"{what}: {name} {list(got[i])[:8]}, oracle {list(want[i])[:8]}"
    assert int(np.asarray(got[2], np.uint64).sum()) == got[0], f"{what}: the counts do not sum to counted"


# ---- the scenarios' CPU side --------------------------------------------------------------------------------------

# tests/test_census.py::scenario_eviction: leave, tombstone and evicted-as-unknown cells
EVICTION_N, EVICTION_ROUNDS, EVICTION_KW = 24, 80, dict(faulty_ms=2000, tombstone_ms=1000)
CASCADE_N, CASCADE_ROUNDS, CASCADE_KILL_ROUND = 300, 40, 3
CASCADE_CHECKED = (2, 5, 27, 28, 29, 30, 31, 32, 33, 39)
# distinct ring checksums (live, all) after the round, computed on the CPU oracle; the server counts are 297..300
CASCADE_DISTINCT = {2: (1, 1), 27: (1, 1), 28: (4, 4), 29: (5, 5), 30: (8, 8), 31: (8, 8), 32: (4, 5), 33: (1, 2),
                    39: (1, 2)}


def eviction_events():
    from swimsim import workloads as W
    return [(0, W.EV_KILL, 3, 0), (2, W.EV_LEAVE, 7, 0), (4, W.EV_KILL, 9, 0), (30, W.EV_REAP, 1, 0),
            (40, W.EV_REVIVE, 3, 0), (41, W.EV_REINCARNATE, 11, 0)]


def cascade_workload():
    from swimsim import workloads as W
    return W.config3(n=CASCADE_N, rounds=CASCADE_ROUNDS, kill_round=CASCADE_KILL_ROUND)
