"""CPU checks of the key-routing boundary: the entry points refuse a NULL handle without writing anything, and the
host-side helpers (swimsim.metrics.route_agreement, the shard merge of route-census histograms) are checked on
hand-made histograms. No device work runs here."""
import ctypes as C

import numpy as np
import pytest

import swimsim
from swimsim import metrics


def test_null_handle_is_refused_and_nothing_is_written():
    L = swimsim.load_library()
    blob, off = swimsim._pack_keys(["a", "bc"])
    obs = np.zeros(1, np.uint32)
    owners = np.full(2, -7, np.int32)
    ms = C.c_double(-1.0)
    assert L.swimsim_route(None, blob, off.ctypes.data, 2, 100, obs.ctypes.data, 1, 0, owners.ctypes.data, C.byref(ms)) == -1
    assert (owners == -7).all() and ms.value == -1.0
    hoff = np.full(3, 77, np.uint64)
    own = np.full(4, -9, np.int32)
    cnt = np.full(4, 9, np.uint32)
    counted, nh = C.c_uint32(123), C.c_size_t(456)
    assert L.swimsim_route_census(None, blob, off.ctypes.data, 2, 100, 0, 0, C.byref(counted), hoff.ctypes.data,
                                  own.ctypes.data, cnt.ctypes.data, 4, C.byref(nh), C.byref(ms)) == -1
    assert (hoff == 77).all() and (own == -9).all() and (cnt == 9).all()
    assert counted.value == 123 and nh.value == 456 and ms.value == -1.0


def test_pack_keys():
    blob, off = swimsim._pack_keys(["ab", b"\x00\xff", "", "xyz"])
    assert blob == b"ab\x00\xffxyz" and list(off) == [0, 2, 4, 4, 7] and off.dtype == np.uint64
    blob, off = swimsim._pack_keys([])
    assert blob == b"" and list(off) == [0]


# key 0: everyone answers 5; key 1: 3 rows answer -1 (empty ring), 4 answer 2, 3 answer 9; key 2: a tie between 4 and 8;
# key 3: a tie between -1 and 0
HIST = (10, [0, 1, 4, 6, 8], [5, -1, 2, 9, 4, 8, -1, 0], [10, 3, 4, 3, 5, 5, 5, 5])


def test_route_agreement():
    ag = metrics.route_agreement(*HIST)
    assert list(ag.distinct) == [1, 3, 2, 2]
    assert list(ag.owner) == [5, 2, 4, -1]                            # plurality; ties go to the lowest owner
    assert list(ag.count) == [10, 4, 5, 5]
    assert list(ag.agreed(10)) == [True, False, False, False]


def test_route_agreement_without_counted_rows():
    ag = metrics.route_agreement(0, [0, 0, 0], [], [])
    assert list(ag.distinct) == [0, 0] and list(ag.owner) == [-2, -2] and list(ag.count) == [0, 0]


def test_route_agreement_refuses_ragged_input():
    with pytest.raises(ValueError):
        metrics.route_agreement(3, [0, 1, 2], [1], [3])
    with pytest.raises(ValueError):
        metrics.route_agreement(3, [0, 1], [1, 2], [3])


def hist(counted, off, own, cnt, ms=0.5):
    return counted, np.array(off, np.uint64), np.array(own, np.int32), np.array(cnt, np.uint32), ms


def test_shard_merge_adds_per_key_and_owner():
    a = hist(4, [0, 1, 3, 4], [7, -1, 3, 2], [4, 1, 3, 4])             # key 0: {7: 4}   key 1: {-1: 1, 3: 3}   key 2: {2: 4}
    b = hist(3, [0, 2, 3, 5], [6, 7, 3, -1, 2], [1, 2, 3, 1, 2])       # key 0: {6: 1, 7: 2}   key 1: {3: 3}   key 2: {-1: 1, 2: 2}
    c = hist(0, [0, 0, 0, 0], [], [])                                   # a shard with no counted row
    counted, off, own, cnt, ms = swimsim.merge_route_histograms([a, b, c])
    assert counted == 7 and ms == 1.5
    assert list(off) == [0, 2, 4, 6] and off.dtype == np.uint64
    assert list(own) == [6, 7, -1, 3, -1, 2] and own.dtype == np.int32
    assert list(cnt) == [1, 6, 1, 6, 1, 6] and cnt.dtype == np.uint32
    ag = metrics.route_agreement(counted, off, own, cnt)
    assert list(ag.owner) == [7, 3, 2] and list(ag.count) == [6, 6, 6] and list(ag.distinct) == [2, 2, 2]


def test_shard_merge_of_one_part_is_that_part():
    a = hist(*HIST)
    counted, off, own, cnt, _ = swimsim.merge_route_histograms([a])
    assert counted == 10 and (off == a[1]).all() and (own == a[2]).all() and (cnt == a[3]).all()
