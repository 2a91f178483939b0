"""Requests forwarded through every node's own ring view (swimsim_forward, swimsim_forward_census) against the CPU oracle.

Every expected value comes from the oracle alone: tests/test_route.py::oracle_owners gives owner(h, k) for every row from
OracleSim.rows(), OracleSim.live() and the partition labels the test set give reach, and tests/forward_cases.py restates
the chain of include/swimsim.h in numpy over them. Equality is exact: every request, every bin, nothing sampled, in modes
0 (production), 1 (ring walk), 2 (direct path) and 3 (an owner table of 8 keys per pass). The figures asserted per
scenario are what the oracle alone gives; they keep a test from passing on a scenario in which nothing happens.
"""
import ctypes as C

import numpy as np
import pytest

import address_scenarios as S
import forward_cases as F
from oracle_ffi import OracleSim, fingerprint32
import swimsim
from swimsim import metrics
from swimsim import workloads as W
from test_census import make_pair, scenario_eviction, scenario_self_only, step_both
from test_route import KEYS64, cascade_keys, oracle_owners

pytestmark = pytest.mark.gpu


def live_of(ora):
    return np.array([ora.live(o) for o in range(ora.n)], bool)


def check(eng, ora, keys, part=None, what="", **kw):
    """check_state over the oracle's state; returns (owners, listed, census) as expected"""
    owners = oracle_owners(ora, keys, kw.get("R", 100), kw.pop("addresses", None))
    part = np.zeros(ora.n, np.int64) if part is None else part
    listed, census = F.check_state(eng, owners, live_of(ora), part, keys, what=what, **kw)
    return owners, listed, census


def totals(census):
    return list(census[1].sum(axis=0))


# ---- 1. scenarios ---------------------------------------------------------------------------------------------------

def test_cascade():
    """W.config3(n=300, kill_round=3), 64 keys, max_hops 8: before the kill every request is served; while the three
    killed members are suspect their keys die at the entry node; while the live nodes drop them one by one (rounds 28 to
    32) a request also dies one hop in, at a node that still holds the dead owner; from round 33 on all is served."""
    wl = W.config3(n=300, rounds=40, kill_round=3)
    keys = cascade_keys(wl)
    eng, ora = make_pair(wl.n)
    try:
        seen = {}
        for r in range(40):
            step_both(eng, ora, wl.events)
            if r in (2, 5) + tuple(range(27, 34)) + (39,):
                _, listed, census = check(eng, ora, keys, what=f"round {r}")
                alive = live_of(ora)
                dead_end = (listed[0][alive] == F.UNREACHABLE)
                seen[r] = (totals(census), int((dead_end & (listed[1][alive] == 0)).sum()), int((dead_end & (listed[1][alive] == 1)).sum()),
                           list(census[2].sum(axis=0)[:3]))
        assert seen[2] == ([64, 19136, 0, 0, 0, 0], 0, 0, [64, 19136, 0])
        assert seen[5] == ([40, 11840, 7128, 0, 0, 0], 7128, 0, [7168, 11840, 0])
        assert seen[30][0][2] == 6445 and seen[30][2] == 1333
        assert seen[33][0][2] == 0 and seen[39][0][2] == 0
        assert eng.digest() == ora.digest()
    finally:
        eng.close()


@pytest.mark.parametrize("max_hops", [8, 1, 64])
def test_leave_bounce(max_hops):
    """scenario_eviction: member 7 leaves at round 2 and still runs. It is no server in its own ring, so it forwards its
    former keys on, and the nodes that have not heard yet send them back: HOP_LIMIT, with hops == max_hops."""
    (eng, ora), events, _ = scenario_eviction()
    try:
        limit = {}
        for r in range(5):
            step_both(eng, ora, events)
            _, listed, census = check(eng, ora, KEYS64, max_hops=max_hops, what=f"max_hops {max_hops} round {r}")
            at_limit = listed[0] == F.HOP_LIMIT
            assert (listed[1][at_limit] == max_hops).all() and (listed[4][at_limit] >= 0).all()
            limit[r] = totals(census)[F.HOP_LIMIT]
        # a bounce never ends: as many at 64 hops as at 8. With one forward allowed the two-hop chains count too
        assert [limit[r] for r in range(5)] == ([0, 0, 78, 56, 0] if max_hops == 1 else [0, 0, 46, 23, 0])
    finally:
        eng.close()


def test_partition():
    """n = 64, members 32..63 in partition 1 from round 0: at first every forward across the cut fails; once both halves
    hold each other faulty every key has two handlers, one per half."""
    n = 64
    eng, ora = make_pair(n)
    part = np.zeros(n, np.int64)
    part[32:] = 1
    events = [(0, W.EV_PARTITION, m, 1) for m in range(32, n)]
    try:
        for r in range(37):
            step_both(eng, ora, events)
            if r in (0, 36):
                _, _, census = check(eng, ora, KEYS64, part=part, what=f"partition round {r}")
                if r == 0:
                    assert totals(census)[F.UNREACHABLE] == 2048 and F.split_keys(census) == 0
        assert totals(census)[F.UNREACHABLE] == 0 and F.split_keys(census) == 64
        assert (np.diff(census[3].astype(np.int64)) == 2).all() and (census[4] >= 0).all()
        av = metrics.forward_availability(*eng.forward_census(KEYS64)[:6])
        assert av.split.all() and av.split_keys == 64 and (av.served == 1.0).all() and av.hops_exact.all()
    finally:
        eng.close()


def test_self_only_start():
    """scenario_self_only (n = 65): rings of 1 to 3 members, chains of two hops, and almost every key served by several
    nodes at once; members 10 and 64 are dead entries."""
    (eng, ora), events, rounds = scenario_self_only()
    try:
        for r in range(rounds):
            step_both(eng, ora, events)
            _, listed, census = check(eng, ora, KEYS64, what=f"self-only round {r}")
            assert (listed[0][[10, 64]] == F.ENTRY_DOWN).all() and (listed[3][10] == 10).all()
            if r == 0:
                assert list(census[2].sum(axis=0)[:3]) == [1106, 1169, 1757] and F.split_keys(census) == 62
        assert census[2].sum(axis=0)[2] == 0, "round 5: no request needs two hops"
    finally:
        eng.close()


def test_crafted_chain():
    """n = 12, one replica point each, one key, self-only start: the member whose point is r-th in clockwise distance
    from the key learns the member of rank r - 1 and nobody else, so a request entering at rank r walks r hops down to
    rank 0."""
    n, key = 12, "key-7"
    eng, ora = make_pair(n, init="self")
    try:
        kh = fingerprint32(key.encode())
        rank = sorted(range(n), key=lambda m: ((fingerprint32((swimsim.address_of(m) + "0").encode()) - kh) % 2 ** 32, m))
        for r in range(1, n):
            assert eng.make_change(rank[r], rank[r - 1], swimsim.T0_MS, swimsim.ALIVE) == \
                ora.make_change(rank[r], rank[r - 1], swimsim.T0_MS, 0)
        owners = oracle_owners(ora, [key], 1)
        assert owners[rank[0], 0] == rank[0] and all(owners[rank[r], 0] == rank[r - 1] for r in range(1, n))
        where = np.argsort(rank)                                       # member -> rank
        for max_hops in (1, 4, 10, 11):
            listed, _ = F.check_state(eng, owners, live_of(ora), np.zeros(n, np.int64), [key], max_hops=max_hops, R=1,
                                      what=f"chain max_hops {max_hops}")
            for m in range(n):
                r = int(where[m])
                if r <= max_hops:
                    assert (listed[0][m, 0], listed[1][m, 0], listed[2][m, 0]) == (F.DELIVERED if r else F.LOCAL, r, rank[0])
                else:
                    assert (listed[0][m, 0], listed[1][m, 0], listed[2][m, 0]) == (F.HOP_LIMIT, max_hops, -1)
                    assert listed[3][m, 0] == rank[r - max_hops] and listed[4][m, 0] == rank[r - max_hops - 1]
            one, _ = F.check_state(eng, owners, live_of(ora), np.zeros(n, np.int64), [key], max_hops=max_hops,
                                   policy=F.ONE_HOP, R=1, what=f"one hop, max_hops {max_hops}")
            for r in range(1, n):
                assert (one[0][rank[r], 0], one[1][rank[r], 0], one[2][rank[r], 0]) == (F.DELIVERED, 1, rank[r - 1])
        assert eng.node(rank[2]).HandleOrForward(key, 8, 1) == (False, swimsim.address_of(rank[0]), "delivered")
        assert eng.node(rank[0]).HandleOrForward(key, 8, 1) == (True, swimsim.address_of(rank[0]), "local")
        assert eng.node(rank[11]).HandleOrForward(key, 8, 1) == (False, "", "hop_limit")
    finally:
        eng.close()


# ---- 2. edge cases --------------------------------------------------------------------------------------------------

def test_no_owner_entry_down_and_duplicates():
    """rows 5 and 69 hold every member faulty: NO_OWNER at hop 0 for the requests that enter there and at hop 1 for the
    key the other nodes send to member 5; member 9 is killed (ENTRY_DOWN, and the requests for its key die UNREACHABLE);
    requests may repeat."""
    n = 70
    eng, ora = make_pair(n)
    try:
        for o in (5, 69):
            for m in range(n):
                eng.set_member(o, m, swimsim.FAULTY, swimsim.T0_MS)
                ora.set_member(o, m, swimsim.FAULTY, swimsim.T0_MS)
        eng.set_live(9, False)
        ora.set_live(9, False)
        owners, listed, census = check(eng, ora, KEYS64, what="no owner / entry down")
        assert (listed[0][[5, 69]] == F.NO_OWNER).all() and (listed[3][5] == 5).all() and (listed[2][5] == -1).all()
        assert (listed[0][9] == F.ENTRY_DOWN).all() and (listed[1][9] == 0).all() and (listed[3][9] == 9).all()
        assert census[0] == 69 and totals(census)[F.NO_OWNER] == 2 * 64 + 67 and totals(census)[F.UNREACHABLE] == 67
        assert ((listed[0] == F.NO_OWNER) & (listed[1] == 1)).sum() == 67
        entries = [5, 9, 9, 3, 69, 3, 3, 0, 68]
        kix = [0, 1, 1, 63, 7, 63, 2, 2, 63]
        want = F.chase(owners, live_of(ora), np.zeros(n, np.int64), entries, kix, 8)
        for mode in F.MODES:
            F.check_listed(eng.forward(KEYS64, entries, kix, mode=mode), want, f"duplicates mode {mode}")
        assert eng.node(5).HandleOrForward(KEYS64[0]) == (False, "", "no_owner")
        assert eng.node(9).HandleOrForward(KEYS64[0]) == (False, "", "entry_down")
    finally:
        eng.close()


def test_single_node():
    eng, ora = make_pair(1)
    try:
        step_both(eng, ora, [])
        _, listed, census = check(eng, ora, KEYS64[:5], what="n=1")
        assert (listed[0] == F.LOCAL).all() and totals(census) == [5, 0, 0, 0, 0, 0]
    finally:
        eng.close()


def test_thirteen_byte_addresses_and_thousand_replica_points():
    n = 40
    addrs = S.addresses(n, 13, 0)
    eng = swimsim.Cluster(n, addresses=addrs)
    try:
        ora = OracleSim(n, addresses=addrs)
        events = [(0, W.EV_KILL, 7, 0)]
        for r in range(3):
            step_both(eng, ora, events)
        _, _, census = check(eng, ora, KEYS64, addresses=addrs, what="W=13")
        assert totals(census)[F.UNREACHABLE] > 0
        check(eng, ora, KEYS64[:20], R=1000, addresses=addrs, what="W=13 R=1000")
        assert eng.node(3).HandleOrForward(KEYS64[0])[1] in ("",) + tuple(addrs)
    finally:
        eng.close()


# ---- 3. paging and chunking -----------------------------------------------------------------------------------------

def mid_cascade():
    wl = W.config3(n=300, rounds=40, kill_round=3)
    eng, ora = make_pair(wl.n)
    eng.step(31, wl.events)
    ora.run(31, wl.events)
    return eng, ora, cascade_keys(wl)


def test_small_cap_returns_the_full_size_and_complete_offsets():
    eng, ora, keys = mid_cascade()
    try:
        want = F.census(oracle_owners(ora, keys), live_of(ora), np.zeros(ora.n, np.int64), 8)
        total = len(want[4])
        assert total > len(keys), "some key has more than one handler entry"
        L = swimsim.load_library()
        blob, koff = swimsim._pack_keys(keys)
        K = len(keys)
        for cap in (0, 1, K, total - 1, total):
            outc, hist = np.full((K, 6), 5, np.uint32), np.full((K, 9), 5, np.uint32)
            hoff = np.full(K + 1, 77, np.uint64)
            mem, cnt = np.full(max(1, cap) + 1, -9, np.int32), np.full(max(1, cap) + 1, 9, np.uint32)
            counted, nh = C.c_uint32(), C.c_size_t()
            rc = L.swimsim_forward_census(eng.h, blob, koff.ctypes.data, K, 100, 8, 0, 0, C.byref(counted), outc.ctypes.data,
                                          hist.ctypes.data, hoff.ctypes.data, mem.ctypes.data if cap else None,
                                          cnt.ctypes.data if cap else None, cap, C.byref(nh), None)
            assert rc == 0 and nh.value == total and counted.value == want[0]
            assert (hoff == want[3]).all() and (outc == want[1]).all() and (hist == want[2]).all()
            assert (mem[:cap] == want[4][:cap]).all() and (cnt[:cap] == want[5][:cap]).all()
            assert (mem[cap:] == -9).all() and (cnt[cap:] == 9).all()     # nothing past cap is written
    finally:
        eng.close()


def test_twenty_keys_in_passes_of_eight():
    """mode 3: the owner table holds 8 keys, so 20 keys take passes of 8, 8 and 4; listed requests of keys from all
    three passes, out of key order"""
    eng, ora, keys = mid_cascade()
    try:
        keys = keys[44:64]
        owners, _, census = check(eng, ora, keys, what="20 keys")
        assert totals(census)[F.UNREACHABLE] > 0
        rng = np.random.default_rng(5)
        entries, kix = rng.integers(0, 300, 500), rng.integers(0, 20, 500)
        want = F.chase(owners, live_of(ora), np.zeros(300, np.int64), entries, kix, 2)
        for mode in F.MODES:
            F.check_listed(eng.forward(keys, entries, kix, 2, "chain", 100, mode), want, f"listed mode {mode}")
        assert eng.forward_times()[0] > 0 and eng.forward_times()[1] > 0 and eng.forward_times()[2] == 0
        eng.forward_census(keys, mode=3)
        assert all(t >= 0 for t in eng.forward_times()) and eng.forward_times()[0] > 0
    finally:
        eng.close()


# ---- 4. non-interference, memory, errors ----------------------------------------------------------------------------

def test_forwarding_changes_nothing():
    eng, ora, keys = mid_cascade()
    try:
        before = (eng.digest(), eng.checksums().copy(), eng.counters(), eng.route_census(keys, "all")[:4])
        for mode in F.MODES:
            eng.forward(keys, list(range(300)), mode=mode)
            eng.forward_census(keys, mode=mode)
        first = eng.memory()
        eng.forward(keys, list(range(300)), policy="one_hop")
        eng.forward_census(keys, max_hops=64)
        assert {k: v for k, v in eng.memory().items() if k != "total"} == {k: v for k, v in first.items() if k != "total"}
        after = eng.route_census(keys, "all")[:4]
        assert eng.digest() == before[0] and (eng.checksums() == before[1]).all() and eng.counters() == before[2]
        assert after[0] == before[3][0] and all((a == b).all() for a, b in zip(after[1:], before[3][1:]))
        wl = W.config3(n=300, rounds=40, kill_round=3)
        for r in range(3):
            step_both(eng, ora, wl.events)
            assert (eng.checksums() == ora.checksums()).all() and eng.digest() == ora.digest()
    finally:
        eng.close()


def test_a_handle_that_never_forwards_holds_what_it_held():
    a, b = swimsim.Cluster(300), swimsim.Cluster(300)
    try:
        a.step(2)
        b.step(2)
        b.forward(KEYS64, [1])
        b.forward_census(KEYS64)
        ma, mb = a.memory(), b.memory()
        assert mb["total"] > ma["total"]
        assert {k: v for k, v in ma.items() if k != "total"} == {k: v for k, v in mb.items() if k != "total"}
    finally:
        a.close()
        b.close()


def test_a_shard_is_refused():
    eng = swimsim.ShardedCluster(64, 2)
    try:
        with pytest.raises(swimsim.SwimsimError, match="EINVAL.*shards"):
            eng.shards[1].forward(KEYS64, [40])
        with pytest.raises(swimsim.SwimsimError, match="EINVAL.*shards"):
            eng.shards[0].forward_census(KEYS64)
        for call in (lambda: eng.forward(KEYS64, [0]), lambda: eng.forward_census(KEYS64), eng.forward_times):
            with pytest.raises(swimsim.SwimsimError, match="shards"):
                call()
        assert eng.route(KEYS64, [40]).shape == (1, 64)
    finally:
        eng.close()


def test_errors_leave_the_next_call_correct():
    n = 40
    eng, ora = make_pair(n)
    try:
        events = [(0, W.EV_KILL, 4, 0)]
        eng.step(4, events)
        ora.run(4, events)
        L = swimsim.load_library()
        blob, koff = swimsim._pack_keys(KEYS64)
        K = len(KEYS64)
        ent = np.arange(n, dtype=np.uint32)
        kix = np.zeros(n, np.uint32)
        out8 = [np.full(n * K, 200, np.uint8) for _ in range(2)]
        out32 = [np.full(n * K, -7, np.int32) for _ in range(3)]
        outc, hist = np.full((K, 6), 5, np.uint32), np.full((K, 65), 5, np.uint32)
        hoff = np.full(K + 1, 77, np.uint64)
        mem, cnt = np.full(4 * K, -9, np.int32), np.full(4 * K, 9, np.uint32)
        counted, nh = C.c_uint32(123), C.c_size_t(456)

        def fwd(keys=blob, off=koff.ctypes.data, nkeys=K, R=100, entry=ent.ctypes.data, key_index=None, nreq=n * K, max_hops=8,
                policy=0, mode=0, outcome=out8[0].ctypes.data, hops=out8[1].ctypes.data):
            return L.swimsim_forward(eng.h, keys, off, nkeys, R, entry, key_index, nreq, max_hops, policy, mode, outcome, hops,
                                     *(o.ctypes.data for o in out32), None)

        def census(keys=blob, off=koff.ctypes.data, nkeys=K, R=100, max_hops=8, policy=0, mode=0, outcomes=outc.ctypes.data,
                   hist_off=hoff.ctypes.data):
            return L.swimsim_forward_census(eng.h, keys, off, nkeys, R, max_hops, policy, mode, C.byref(counted), outcomes,
                                            hist.ctypes.data, hist_off, mem.ctypes.data, cnt.ctypes.data, len(mem),
                                            C.byref(nh), None)

        owners = oracle_owners(ora, KEYS64)

        def refused(call, **bad):
            """the call is refused with nothing written, and the next call is correct"""
            assert call(**bad) == -1, f"{call.__name__}({bad}) was not refused"
            assert all((o == 200).all() for o in out8) and all((o == -7).all() for o in out32)
            assert (outc == 5).all() and (hist == 5).all() and (hoff == 77).all() and (mem == -9).all() and (cnt == 9).all()
            assert counted.value == 123 and nh.value == 456
            F.check_state(eng, owners[:, :3], live_of(ora), np.zeros(n, np.int64), KEYS64[:3], what=f"after {call.__name__}({bad})")

        bad_entry, bad_key = ent.copy(), kix.copy()
        bad_entry[7], bad_key[n - 1] = n, K
        for bad in (dict(keys=None), dict(off=None), dict(outcome=None), dict(hops=None), dict(nkeys=0), dict(R=0), dict(R=1001),
                    dict(max_hops=0), dict(max_hops=65), dict(policy=2), dict(policy=-1), dict(mode=4), dict(mode=-1),
                    dict(entry=None), dict(nreq=0), dict(nreq=n * K - 1), dict(entry=bad_entry.ctypes.data),
                    dict(entry=bad_entry.ctypes.data, key_index=kix.ctypes.data, nreq=n),
                    dict(key_index=bad_key.ctypes.data, nreq=n)):
            refused(fwd, **bad)
        for bad in (dict(keys=None), dict(off=None), dict(hist_off=None), dict(outcomes=None), dict(nkeys=0), dict(R=0),
                    dict(R=1001), dict(mode=4), dict(mode=-1), dict(policy=2), dict(max_hops=0), dict(max_hops=65)):
            refused(census, **bad)
        with pytest.raises(ValueError):
            eng.forward_census(KEYS64, policy="twice")
        with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
            eng.forward(KEYS64, [])
        with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
            eng.forward([], [0])
        check(eng, ora, KEYS64, what="after the errors")
    finally:
        eng.close()
