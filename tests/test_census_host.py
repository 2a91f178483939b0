"""CPU checks of the member census boundary: the entry points refuse a NULL handle without touching the device, and
swimsim.metrics.detection_times on hand-made trace arrays."""
import ctypes
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "ringpop-go_amd", "swimsim", "libswimsim.so")


def test_census_entry_points_reject_a_null_handle_without_touching_device():
    import swimsim
    L = swimsim.load_library(LIB)
    counts = (ctypes.c_uint32 * 48)()
    idx = (ctypes.c_uint32 * 2)(0, 1)
    n, dropped = ctypes.c_size_t(7), ctypes.c_uint32(7)
    assert L.swimsim_census(None, None, 8, swimsim.CENSUS_LIVE, counts, None, None, None) == -1
    assert L.swimsim_census(None, idx, 2, swimsim.CENSUS_ALL, counts, None, None, None) == -1
    assert L.swimsim_trace_members(None, idx, 2, 16) == -1
    assert L.swimsim_trace_members(None, None, 0, 0) == -1
    assert L.swimsim_trace_read(None, None, None, None, 0, ctypes.byref(n), ctypes.byref(dropped)) == -1
    assert (n.value, dropped.value) == (7, 7)                       # nothing written
    assert list(counts) == [0] * 48


def counts_of(rows):
    """counts[k, n, 6] from rows[k][n] = {status column: observers}"""
    out = np.zeros((len(rows), len(rows[0]), 6), np.uint32)
    for k, members in enumerate(rows):
        for j, cell in enumerate(members):
            for s, c in cell.items():
                out[k, j, s] = c
    return out


def test_detection_times_on_hand_made_arrays():
    from swimsim import metrics as M
    A, S, F, L, T, U = range(6)
    rounds = [0, 1, 2, 3, 4]
    nlive = [4, 4, 3, 3, 3]
    rows = [
        # member 0: never suspected; 1: suspect in round 1, faulty from 3, everywhere in 4; 2: suspect and faulty in
        # the same round (2), then forgotten by every node (all unknown = detected) in 3; 3: tombstone counts as
        # faulty or worse, leave too
        [{A: 4}, {A: 4}, {A: 4}, {A: 4}],
        [{A: 4}, {A: 3, S: 1}, {A: 4}, {A: 3, L: 1}],
        [{A: 3}, {S: 3}, {A: 1, S: 1, F: 1}, {L: 1, T: 2}],
        [{A: 3}, {S: 2, F: 1}, {U: 3}, {T: 3}],
        [{A: 3}, {F: 3}, {U: 3}, {T: 2, U: 1}],
    ]
    t = M.detection_times(rounds, nlive, counts_of(rows))
    assert t.first_suspect == [None, 1, 2, 1]
    assert t.first_faulty == [None, 3, 2, 1]
    assert t.all_faulty == [None, 4, 3, 2]


def test_detection_times_reports_recorded_rounds_across_a_gap():
    from swimsim import metrics as M
    A, S, F, U = 0, 1, 2, 5
    rounds = [0, 1, 9, 10]                                           # rounds 2..8 were dropped by a full buffer
    nlive = [2, 2, 2, 0]
    rows = [[{A: 2}, {A: 2}], [{A: 2}, {A: 2}], [{S: 1, F: 1}, {A: 2}], [{}, {}]]
    t = M.detection_times(np.array(rounds, np.uint32), np.array(nlive, np.uint32), counts_of(rows))
    assert t.first_suspect == [9, None] and t.first_faulty == [9, None]
    assert t.all_faulty == [None, None]                              # (a round with no live observer detects nothing)
    empty = M.detection_times([], [], np.zeros((0, 3, 6), np.uint32))
    assert empty.first_suspect == [None] * 3 and empty.all_faulty == [None] * 3
    with pytest.raises(ValueError):
        M.detection_times([0], [1], np.zeros((1, 2, 5)))
