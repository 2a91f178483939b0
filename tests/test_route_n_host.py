"""Host-side parts of the replica-set calls (swimsim_route_n, swimsim_replica_census): no device is needed.

replica_agreement on hand-written histograms, the per-(key, member) histogram merge of a sharded census, the Python-side
bound on n, and the binding of the header's two symbols.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import swimsim
from swimsim import metrics

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "swimsim.h")
LIB = os.path.join(REPO, "ringpop-go_amd", "swimsim", "libswimsim.so")


def hist(per_key):
    """(hist_off, hist_member, hist_count) of [[(member, count), ...] per key]"""
    off = np.cumsum([0] + [len(e) for e in per_key]).astype(np.uint64)
    mem = np.array([m for e in per_key for m, _ in e], np.int32)
    cnt = np.array([c for e in per_key for _, c in e], np.uint32)
    return off, mem, cnt


def test_replica_agreement_on_hand_written_histograms():
    # 10 counted rows, n = 3. key 0: all agree on {2, 5, 9}. key 1: 4 rows answer 7 where 6 answer 5: {2, 9} unanimous.
    # key 2: no entry (every counted view is empty). key 3: views of two servers, all agree. key 4: nothing in common.
    off, mem, cnt = hist([[(2, 10), (5, 10), (9, 10)], [(2, 10), (5, 6), (7, 4), (9, 10)], [], [(0, 10), (1, 10)],
                          [(1, 5), (2, 5), (3, 5), (4, 5), (5, 5), (6, 5)]])
    ag = metrics.replica_agreement(10, off, mem, cnt, 3)
    assert list(ag.distinct) == [3, 4, 0, 2, 6]
    assert list(ag.unanimous) == [3, 2, 0, 2, 0]
    assert list(ag.agreed) == [True, False, True, True, False]
    assert ag.agreed.dtype == bool
    # no row counted: no entries, every key agreed
    ag = metrics.replica_agreement(0, np.zeros(4, np.uint64), [], [], 16)
    assert list(ag.distinct) == [0, 0, 0] and ag.agreed.all()


def test_replica_agreement_refuses_what_is_no_replica_census():
    off, mem, cnt = hist([[(2, 10), (5, 10)]])
    with pytest.raises(ValueError):
        metrics.replica_agreement(10, off, mem, cnt[:1], 3)          # lengths differ
    with pytest.raises(ValueError):
        metrics.replica_agreement(10, off[:1], mem, cnt, 3)          # hist_off does not end at the entries
    with pytest.raises(ValueError):
        metrics.replica_agreement(9, off, mem, cnt, 3)               # a count above counted
    with pytest.raises(ValueError):
        metrics.replica_agreement(10, off, mem, cnt, 1)              # two unanimous members in sets of one
    for n in (0, 17):
        with pytest.raises(ValueError):
            metrics.replica_agreement(10, off, mem, cnt, n)


def test_histograms_merge_per_key_and_member():
    a = (4,) + hist([[(1, 4), (3, 4), (8, 4)], [(0, 2), (2, 4), (5, 2)], []]) + (0.5,)
    b = (3,) + hist([[(1, 3), (3, 1), (7, 2), (8, 3)], [(2, 3), (5, 3)], []]) + (0.25,)
    counted, off, mem, cnt, ms = swimsim.merge_route_histograms([a, b])
    assert counted == 7 and ms == 0.75
    assert list(off) == [0, 4, 7, 7]
    assert list(mem) == [1, 3, 7, 8, 0, 2, 5] and list(cnt) == [7, 5, 2, 7, 2, 7, 5]
    assert mem.dtype == np.int32 and cnt.dtype == np.uint32 and off.dtype == np.uint64
    ag = metrics.replica_agreement(counted, off, mem, cnt, 3)
    assert list(ag.unanimous) == [2, 1, 0] and list(ag.agreed) == [False, False, True]


@pytest.mark.parametrize("cls", [swimsim.Cluster, swimsim.ShardedCluster])
@pytest.mark.parametrize("n", [0, 17, -1, 2.5, True])
def test_n_outside_1_to_16_is_refused_before_the_library_is_called(cls, n):
    c = object.__new__(cls)                                           # no handle: a library call would fail otherwise
    with pytest.raises(ValueError, match="1..16"):
        c.route_n(["k"], [0], n)
    with pytest.raises(ValueError, match="1..16"):
        c.replica_census(["k"], n)
    assert swimsim.ROUTE_N_REPLICAS == 16


def test_header_symbols_are_exported_and_bound():
    text = open(HEADER).read()
    assert int(re.search(r"#define SWIMSIM_ABI_VERSION (\d+)", text).group(1)) >= 10
    L = swimsim.load_library(LIB)
    for name in ("swimsim_route_n", "swimsim_replica_census"):
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in swimsim.h"
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and f.argtypes is not None
    assert len(L.swimsim_route_n.argtypes) == 12 and len(L.swimsim_replica_census.argtypes) == 15
    assert L.swimsim_route_n(None, None, None, 0, 100, 3, None, 0, 0, None, None, None) == -1      # no handle: EINVAL
    assert hasattr(swimsim.Node, "LookupN") and hasattr(swimsim.ShardedCluster, "replica_census")
