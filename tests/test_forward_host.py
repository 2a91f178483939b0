"""CPU checks of the forwarding boundary: the header and the bindings, the refusal of a NULL handle without writing
anything, the numpy restatement of the chain (tests/forward_cases.py) on a hand-computed three-node case, and
swimsim.metrics.forward_availability on hand-made histograms. No device work runs here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import forward_cases as F
import swimsim
from swimsim import metrics

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swimsim.h")


def test_header_and_bindings():
    text = open(HEADER).read()
    assert int(re.search(r"#define SWIMSIM_ABI_VERSION (\d+)", text).group(1)) >= 16
    for name, nargs in (("swimsim_forward", 17), ("swimsim_forward_census", 17), ("swimsim_forward_times", 4)):
        proto = re.search(rf"\bint {name}\(([^;]*)\);", text)
        assert proto and len(proto.group(1).split(",")) == nargs, name
        assert len(getattr(swimsim.load_library(), name).argtypes) == nargs
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"SWIMSIM_FWD_(\w+) = (\d+)", text)}
    assert codes == {"LOCAL": 0, "DELIVERED": 1, "UNREACHABLE": 2, "HOP_LIMIT": 3, "NO_OWNER": 4, "ENTRY_DOWN": 5, "CHAIN": 0,
                     "ONE_HOP": 1}
    assert [codes[n.upper()] for n in swimsim.FWD_OUTCOMES] == list(range(6))
    assert (F.LOCAL, F.DELIVERED, F.UNREACHABLE, F.HOP_LIMIT, F.NO_OWNER, F.ENTRY_DOWN) == tuple(range(6))
    assert swimsim.FWD_POLICY == {"chain": F.CHAIN, "one_hop": F.ONE_HOP} and swimsim.FWD_MAX_HOPS == 64


def test_null_handle_is_refused_and_nothing_is_written():
    L = swimsim.load_library()
    keys, off = b"key-0", np.array([0, 5], np.uint64)
    ent = np.zeros(1, np.uint32)
    out8 = [np.full(2, 77, np.uint8) for _ in range(2)]
    out32 = [np.full(2, -7, np.int32) for _ in range(3)]
    ms = C.c_double(-1.0)
    assert L.swimsim_forward(None, keys, off.ctypes.data, 1, 100, ent.ctypes.data, None, 1, 8, 0, 0, *(o.ctypes.data for o in out8),
                             *(o.ctypes.data for o in out32), C.byref(ms)) == -1
    assert all((o == 77).all() for o in out8) and all((o == -7).all() for o in out32) and ms.value == -1.0
    bins = [np.full(9, 5, np.uint32) for _ in range(2)]
    hoff = np.full(2, 77, np.uint64)
    mem, cnt = np.full(4, -9, np.int32), np.full(4, 9, np.uint32)
    counted, nh = C.c_uint32(321), C.c_size_t(456)
    assert L.swimsim_forward_census(None, keys, off.ctypes.data, 1, 100, 8, 0, 0, C.byref(counted), bins[0].ctypes.data,
                                    bins[1].ctypes.data, hoff.ctypes.data, mem.ctypes.data, cnt.ctypes.data, 4, C.byref(nh),
                                    C.byref(ms)) == -1
    assert all((b == 5).all() for b in bins) and (hoff == 77).all() and (mem == -9).all() and (cnt == 9).all()
    assert counted.value == 321 and nh.value == 456 and ms.value == -1.0
    t = [C.c_double(-2.0) for _ in range(3)]
    assert L.swimsim_forward_times(None, *(C.byref(x) for x in t)) == -1 and all(x.value == -2.0 for x in t)


def test_sharded_cluster_names_the_limitation():
    sc = swimsim.ShardedCluster.__new__(swimsim.ShardedCluster)          # (no device: only the refusal is called)
    for call in (lambda: sc.forward(["k"], [0]), lambda: sc.forward_census(["k"]), sc.forward_times):
        with pytest.raises(swimsim.SwimsimError, match="EINVAL.*chains that cross shards"):
            call()


# ---- the restatement on a three-node case worked by hand ----
#
# Nodes 0, 1, 2; keys a, b, c, d. owners[h][k] by the views:
#            a   b   c   d
#   node 0   0   1   1   2
#   node 1   0   1   2   2
#   node 2   0   1   0  -1
# Key a: everybody sends it to 0, which handles it. Key b: 1 handles it. Key c: 0 -> 1 -> 2 -> 0 -> ... never settles.
# Key d: 0 and 1 send it to 2, whose ring is empty.
OWNERS = np.array([[0, 1, 1, 2], [0, 1, 2, 2], [0, 1, 0, -1]])
ALL_LIVE, ONE_PART = np.ones(3, bool), np.zeros(3, int)


def rows(res):
    """the five arrays as tuples (outcome, hops, handler, holder, next) per request"""
    return [tuple(int(a[i]) for a in res) for i in range(len(res[0]))]


def test_restatement_on_three_nodes():
    every = ([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2], [0, 1, 2, 3] * 3)
    got = rows(F.chase(OWNERS, ALL_LIVE, ONE_PART, *every, max_hops=2))
    assert got == [
        (F.LOCAL, 0, 0, 0, -1), (F.DELIVERED, 1, 1, 1, -1), (F.HOP_LIMIT, 2, -1, 2, 0), (F.NO_OWNER, 1, -1, 2, -1),
        (F.DELIVERED, 1, 0, 0, -1), (F.LOCAL, 0, 1, 1, -1), (F.HOP_LIMIT, 2, -1, 0, 1), (F.NO_OWNER, 1, -1, 2, -1),
        (F.DELIVERED, 1, 0, 0, -1), (F.DELIVERED, 1, 1, 1, -1), (F.HOP_LIMIT, 2, -1, 1, 2), (F.NO_OWNER, 0, -1, 2, -1)]
    # one forward allowed: key c stops one node earlier
    assert rows(F.chase(OWNERS, ALL_LIVE, ONE_PART, [0, 2], [2, 2], max_hops=1)) == [(F.HOP_LIMIT, 1, -1, 1, 2), (F.HOP_LIMIT, 1, -1, 0, 1)]
    # ONE_HOP: the first forward delivers, whatever the destination's own view says
    assert rows(F.chase(OWNERS, ALL_LIVE, ONE_PART, [0, 0, 2], [2, 3, 0], max_hops=2, policy=F.ONE_HOP)) == \
        [(F.DELIVERED, 1, 1, 1, -1), (F.DELIVERED, 1, 2, 2, -1), (F.DELIVERED, 1, 0, 0, -1)]
    # node 1 dead: it is no entry, and a forward to it fails at the holder
    live = np.array([True, False, True])
    assert rows(F.chase(OWNERS, live, ONE_PART, [1, 0, 2, 0], [0, 1, 1, 0], max_hops=2)) == \
        [(F.ENTRY_DOWN, 0, -1, 1, -1), (F.UNREACHABLE, 0, -1, 0, 1), (F.UNREACHABLE, 0, -1, 2, 1), (F.LOCAL, 0, 0, 0, -1)]
    # node 2 in another partition: key c gets from 0 to 1 and fails there
    part = np.array([0, 0, 1])
    assert rows(F.chase(OWNERS, ALL_LIVE, part, [0, 2, 2], [2, 2, 3], max_hops=2)) == \
        [(F.UNREACHABLE, 1, -1, 1, 2), (F.UNREACHABLE, 0, -1, 2, 0), (F.NO_OWNER, 0, -1, 2, -1)]


def test_restated_census_on_three_nodes():
    counted, outcomes, hist, off, mem, cnt = F.census(OWNERS, ALL_LIVE, ONE_PART, 2)
    assert counted == 3
    assert outcomes.tolist() == [[1, 2, 0, 0, 0, 0], [1, 2, 0, 0, 0, 0], [0, 0, 0, 3, 0, 0], [0, 0, 0, 0, 3, 0]]
    assert hist.tolist() == [[1, 2, 0], [1, 2, 0], [0, 0, 3], [1, 2, 0]]
    assert off.tolist() == [0, 1, 2, 3, 4] and mem.tolist() == [0, 1, -1, -1] and cnt.tolist() == [3, 3, 3, 3]
    assert F.split_keys((counted, outcomes, hist, off, mem, cnt)) == 0
    grid = F.chase_grid(OWNERS, ALL_LIVE, ONE_PART, [2, 0], 2)
    assert grid[0].shape == (2, 4) and grid[2].tolist() == [[0, 1, -1, -1], [0, 1, -1, -1]]
    # node 1 alone in its partition: it keeps key b for itself, nobody else reaches it
    counted, outcomes, hist, off, mem, cnt = F.census(OWNERS, ALL_LIVE, np.array([0, 1, 0]), 2)
    assert outcomes[1].tolist() == [1, 0, 2, 0, 0, 0] and mem[off[1]:off[2]].tolist() == [-1, 1] and cnt[off[1]:off[2]].tolist() == [2, 1]
    assert F.census(OWNERS, np.zeros(3, bool), ONE_PART, 2)[0] == 0


# ---- forward_availability on hand-made histograms ----

def test_forward_availability():
    # 10 entries, max_hops 2. key 0: all served, 4 local and 6 after one hop, one handler. key 1: split between nodes 3
    # (7 entries, one of them local) and 8 (3 entries, two hops each). key 2: nobody serves it: 6 unreachable at hop 0
    # and 4 at the hop limit. key 3: 5 served after one hop, 5 unreachable at hop 1
    outcomes = [[4, 6, 0, 0, 0, 0], [1, 9, 0, 0, 0, 0], [0, 0, 6, 4, 0, 0], [0, 5, 5, 0, 0, 0]]
    hops = [[4, 6, 0], [1, 6, 3], [6, 0, 4], [0, 10, 0]]
    off, handler, count = [0, 1, 3, 4, 6], [5, 3, 8, -1, -1, 2], [10, 7, 3, 10, 5, 5]
    av = metrics.forward_availability(10, outcomes, hops, off, handler, count)
    assert av.served.tolist() == [1.0, 1.0, 0.0, 0.5]
    assert av.mean_hops[0] == pytest.approx(0.6) and av.mean_hops[1] == pytest.approx(1.2) and np.isnan(av.mean_hops[2])
    assert av.mean_hops[3] == pytest.approx(2.0) and av.hops_exact.tolist() == [True, True, False, False]   # (key 3: an upper bound)
    assert av.handlers.tolist() == [1, 2, 0, 1] and av.split.tolist() == [False, True, False, False] and av.split_keys == 1
    assert av.requests == 40 and av.served_total == 25
    assert av.outcome_totals.tolist() == [5, 20, 11, 4, 0, 0] and av.hops_total.tolist() == [11, 22, 7]
    none = metrics.forward_availability(0, np.zeros((2, 6)), np.zeros((2, 3)), [0, 0, 0], [], [])
    assert none.served.tolist() == [0.0, 0.0] and np.isnan(none.mean_hops).all() and none.requests == 0 and none.split_keys == 0


def test_forward_availability_refuses_inconsistent_input():
    good = dict(counted=4, outcomes=[[1, 3, 0, 0, 0, 0]], hops_hist=[[1, 3]], hist_off=[0, 1], hist_handler=[2], hist_count=[4])
    metrics.forward_availability(**good)
    for bad in (dict(outcomes=[[1, 2, 0, 0, 0, 0]]), dict(hops_hist=[[1, 2]]), dict(hist_count=[3]), dict(hist_off=[0, 2]),
                dict(hist_handler=[-1]), dict(outcomes=[[1, 3, 0, 0, 0]]), dict(hops_hist=[[4]])):
        with pytest.raises(ValueError):
            metrics.forward_availability(**dict(good, **bad))
