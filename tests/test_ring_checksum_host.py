"""CPU checks of the ring-checksum boundary: the tests' expectation helper against the oracle's ring, the two known
answers, the header and the bindings, the refusal of a NULL handle without writing anything, and the host-side helpers
(swimsim.metrics.ring_agreement, the shard merge of ring-census histograms) on hand-made histograms. No device work runs
here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle_ffi import OracleRing, OracleSim, fingerprint32
import ring_checksum_scenarios as RS
import swimsim
from swimsim import metrics

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swimsim.h")


def oracle_ring_checksum(addr, present):
    ring = OracleRing(100)
    ring.add_remove_servers([addr[m] for m in np.nonzero(present)[0]], [])
    return ring.checksum()


def check_helper_against_ring(ora, seen, what):
    addr = RS.addresses_of(ora.n)
    st = ora.rows()[0]
    cs, srv, _ = RS.expected(ora)
    for o in range(ora.n):
        present = st[o] <= 1
        key = present.tobytes()
        if key in seen:
            assert cs[o] == seen[key]
            continue
        seen[key] = oracle_ring_checksum(addr, present)
        assert cs[o] == seen[key], f"{what}: row {o} of {int(present.sum())} servers"
        assert srv[o] == present.sum()


def test_helper_equals_oracle_ring_on_the_eviction_views():
    ora = OracleSim(RS.EVICTION_N, **RS.EVICTION_KW)
    events, seen = RS.eviction_events(), {}
    for r in range(RS.EVICTION_ROUNDS):
        ora.step([e for e in events if e[0] == r])
        check_helper_against_ring(ora, seen, f"eviction round {r}")
    assert len(seen) >= 4 and len({int(np.frombuffer(k, bool).sum()) for k in seen}) >= 3


def test_helper_equals_oracle_ring_on_the_cascade_views_and_their_distinct_counts():
    wl = RS.cascade_workload()
    ora = OracleSim(wl.n)
    seen = {}
    for r in range(wl.rounds):
        ora.step([e for e in wl.events if e[0] == r])
        if r not in RS.CASCADE_CHECKED:
            continue
        check_helper_against_ring(ora, seen, f"cascade round {r}")
        cs, srv, _ = RS.expected(ora)
        assert 297 <= srv.min() and srv.max() <= 300
        if r in RS.CASCADE_DISTINCT:
            got = tuple(len(np.unique(cs[RS.live_mask(ora, who)])) for who in ("live", "all"))
            assert got == RS.CASCADE_DISTINCT[r], f"round {r}: distinct ring checksums {got}"


def test_known_answers():
    assert fingerprint32(b"") == RS.EMPTY == swimsim.EMPTY_RING_CHECKSUM
    addr = [swimsim.address_of(m) for m in range(5)]
    ring = OracleRing(100)
    ring.add_remove_servers(addr[::-1], [])                            # added in reverse: the checksum sorts
    assert ring.checksum() == RS.MEMBERS_0_TO_4
    assert RS.view_checksum(addr, np.ones(5, bool)) == RS.MEMBERS_0_TO_4
    cs, srv, views = RS.expected_rows(np.array([[0, 1, 0, 1, 0], [7, 2, 3, 4, 7], [0, 0, 1, 1, 0]]))
    assert list(cs) == [RS.MEMBERS_0_TO_4, RS.EMPTY, RS.MEMBERS_0_TO_4] and list(srv) == [5, 0, 5] and views == 2


def test_header_and_bindings():
    text = open(HEADER).read()
    assert int(re.search(r"#define SWIMSIM_ABI_VERSION (\d+)", text).group(1)) >= 15
    for name in ("swimsim_ring_checksums", "swimsim_ring_census"):
        assert re.search(rf"\bint {name}\(", text), name
    L = swimsim.load_library()
    assert len(L.swimsim_ring_checksums.argtypes) == 8
    assert len(L.swimsim_ring_census.argtypes) == 12
    assert swimsim.RING_CHECKSUM_CHUNK >= 256 and swimsim.RING_CHECKSUM_CHUNK % 256 == 0


def test_null_handle_is_refused_and_nothing_is_written():
    L = swimsim.load_library()
    obs = np.zeros(1, np.uint32)
    cs = np.full(2, 77, np.uint32)
    srv = np.full(2, 78, np.uint32)
    hashed, ms = C.c_uint32(123), C.c_double(-1.0)
    assert L.swimsim_ring_checksums(None, obs.ctypes.data, 1, 0, cs.ctypes.data, srv.ctypes.data, C.byref(hashed),
                                    C.byref(ms)) == -1
    assert (cs == 77).all() and (srv == 78).all() and hashed.value == 123 and ms.value == -1.0
    bufs = [np.full(4, 9 + i, np.uint32) for i in range(4)]
    counted, nh = C.c_uint32(321), C.c_size_t(456)
    assert L.swimsim_ring_census(None, 0, 0, C.byref(counted), *(b.ctypes.data for b in bufs), 4, C.byref(nh),
                                 C.byref(hashed), C.byref(ms)) == -1
    assert all((b == 9 + i).all() for i, b in enumerate(bufs))
    assert counted.value == 321 and nh.value == 456 and hashed.value == 123 and ms.value == -1.0


# ---- pure Python: ring_agreement and the shard merge ----

def test_ring_agreement():
    ag = metrics.ring_agreement(10, [5, 900, 4000000000], [3, 4, 3])
    assert (ag.distinct, ag.checksum, ag.all_agree) == (3, 900, False) and ag.share == pytest.approx(0.4)
    ag = metrics.ring_agreement(10, [5, 900], [5, 5])                  # a tie goes to the lowest checksum
    assert (ag.distinct, ag.checksum, ag.share, ag.all_agree) == (2, 5, 0.5, False)
    ag = metrics.ring_agreement(7, [RS.EMPTY], [7])
    assert (ag.distinct, ag.checksum, ag.share, ag.all_agree) == (1, RS.EMPTY, 1.0, True)
    ag = metrics.ring_agreement(0, [], [])
    assert (ag.distinct, ag.checksum, ag.share, ag.all_agree) == (0, None, 0.0, False)


def test_ring_agreement_refuses_inconsistent_input():
    with pytest.raises(ValueError):
        metrics.ring_agreement(3, [1, 2], [3])
    with pytest.raises(ValueError):
        metrics.ring_agreement(4, [1, 2], [1, 2])                      # the counts do not sum to counted
    with pytest.raises(ValueError):
        metrics.ring_agreement(3, [2, 1], [1, 2])                      # not ascending


def part(counted, cs, cnt, srv, first, hashed=1, ms=0.5):
    return (counted, np.array(cs, np.uint32), np.array(cnt, np.uint32), np.array(srv, np.uint32), np.array(first, np.uint32),
            hashed, ms)


def test_shard_merge_adds_per_checksum_and_keeps_the_lowest_first_row():
    a = part(5, [10, 4000000000], [4, 1], [300, 299], [0, 3], hashed=2)
    b = part(4, [7, 10, 4000000000], [1, 2, 1], [298, 300, 299], [105, 100, 101], hashed=3)
    c = part(0, [], [], [], [], hashed=0)                               # a shard with no counted row
    # equal checksums of different views (a collision): first and servers come from the lower first row, shard d's
    d = part(2, [10], [2], [297], [200], hashed=1)
    counted, cs, cnt, srv, first, hashed, ms = swimsim.merge_ring_histograms([b, d, a, c])
    assert counted == 11 and hashed == 6 and ms == 2.0
    assert list(cs) == [7, 10, 4000000000] and cs.dtype == np.uint32
    assert list(cnt) == [1, 8, 2] and list(first) == [105, 0, 3] and list(srv) == [298, 300, 299]
    ag = metrics.ring_agreement(counted, cs, cnt)
    assert ag.distinct == 3 and ag.checksum == 10 and not ag.all_agree
    d2 = part(2, [10], [2], [297], [0], hashed=1)                       # now the other view holds the lowest row
    a2 = part(5, [10, 4000000000], [4, 1], [300, 299], [1, 3], hashed=2)
    _, cs, cnt, srv, first, _, _ = swimsim.merge_ring_histograms([a2, d2])
    assert list(cs) == [10, 4000000000] and list(cnt) == [6, 1] and list(first) == [0, 3] and list(srv) == [297, 299]


def test_shard_merge_of_one_part_is_that_part():
    a = part(5, [10, 4000000000], [4, 1], [300, 299], [0, 3], hashed=2)
    got = swimsim.merge_ring_histograms([a])
    assert got[0] == 5 and all((got[i] == a[i]).all() for i in range(1, 5)) and got[5] == 2
    assert swimsim.merge_ring_histograms([part(0, [], [], [], [], hashed=0)])[:1] == (0,)
