"""What the view checkpoints of tests/test_fuzz_views.py hold, on the CPU oracle alone: the committed schedules
(fuzz_scenarios.case, n >= 5) run as tests/test_fuzz.py runs their oracle side, and at every checkpoint
(fuzz_views.checkpoint_calls) the expectations an engine would be compared with are computed and noted
(fuzz_views.expected_views: 64 keys, R = 100, chain policy, 8 hops). The assertions are conditions on the input: a later
change to the schedules cannot quietly leave the view tests with tidy states. No device work runs here.

Measured over the 24 cases (the 21 of up to 130 members, which the tests without the `slow` mark take, and the three of
257): 489 checkpoints (467 + 22) and 44,037 rows, 4,276 of them of dead observers; 121 empty views, 3,909 of 1 to 3
servers, 201 of 4 to 16 (all three classes in the cases up to 130) and 39,806 of more than 16; up to 127 distinct views
among 127 rows and 256 among the 257 of case 257-0, whose live rows answer up to 233 ring checksums; all six cell values
in every case; census minimum and maximum differ for a member 24,396 times, by up to 87 periods; forward-census outcomes
local 232,860, delivered 2,117,366, unreachable 177,738, hop_limit 11,246 (in every case of 63 to 130 members and in 257-0), no_owner
5,494 (cases 5-0, 5-1, 5-2, 64-1, 64-2, 65-0, 65-2 and 127-1); 273,664 entry_down requests in the listed calls; 12,021
split keys and 20,722 disagreeing keys, up to all 64 at one checkpoint, and 24,290 (checkpoint, key) pairs whose
replica sets at n = 3 disagree among the live rows. At 1,100 members (case 1100-0): 37 dead rows, 367 members behind the
cut and 795 distinct views after the call that holds round 8, 26 dead rows and 24 views at the end; the chains of the 48
sampled entries visit 63 and 76 rows."""
import numpy as np
import pytest

import forward_cases as FC
import fuzz_scenarios as F
import fuzz_views as V
from oracle_ffi import OracleSim

SMALL = [(n, s) for n, s in V.CASES if n <= V.EVERY_CALL_UP_TO]
LARGE = [(n, s) for n, s in V.CASES if n > V.EVERY_CALL_UP_TO]


def run_checkpoints(c, reach):
    """case c on the oracle; expected_views at every checkpoint, and the tracker's liveness against the oracle's"""
    n = c["n"]
    ora = OracleSim(n, init=c["init"], **c["options"])
    tracker = V.Tracker(n)
    checked = V.checkpoint_calls(c)
    for i, call in enumerate(c["calls"]):
        F.oracle_call(ora, call)
        tracker.apply(call)
        assert [ora.live(o) for o in range(n)] == list(tracker.live), f"case {n}-{c['seed']}: liveness after call {i}"
        if i in checked:
            V.expected_views(ora, tracker.part, V.KEYS64, R=100, reach=reach)
    return ora


def reach_of(cases):
    per_case = {}
    for n, seed in cases:
        per_case[(n, seed)] = V.new_reach()
        run_checkpoints(F.case(n, seed), per_case[(n, seed)])
    return per_case


@pytest.fixture(scope="module")
def small():
    return reach_of(SMALL)


@pytest.fixture(scope="module")
def large():
    return reach_of(LARGE)


def total(per_case, key):
    return sum(r[key] for r in per_case.values())


def test_checkpoints():
    assert len(V.CASES) == 24 and len(SMALL) == 21 and [n for n, _ in LARGE] == [257] * 3
    for n, seed in V.CASES:
        c = F.case(n, seed)
        k = len(c["calls"])
        want = set(range(k)) if n <= 130 else {i for i in range(k) if i % 4 == 0 or i == k - 1}
        assert V.checkpoint_calls(c) == want
    assert V.traced_members(5) == [0, 1, 2, 3, 4] and V.traced_members(64) == list(range(64))
    assert V.traced_members(65) == list(range(0, 65, 2)) and len(V.traced_members(257)) == 52
    assert all(len(V.traced_members(n)) <= 64 for n in F.SIZES)
    for n in (5, 63, 257):
        short, long = V.duplicate_lists(n)
        assert len(set(short)) < len(short) and len(set(long)) < len(long) and max(long) < n
        assert 16 * len(short) <= 64 and (n < 63 or 16 * len(long) > -(-n // 64) * 64)


def test_tracker_follows_mutators_then_events():
    t = V.Tracker(4)
    t.apply({"muts": [("set_partition", 1, 2), ("set_live", 2, False), ("heal", 0)],
             "events": [(0, F.EV_PARTITION, 1, 1), (0, F.EV_KILL, 3, 0), (1, F.EV_REVIVE, 2, 0), (1, F.EV_LEAVE, 0, 0)]})
    assert list(t.part) == [0, 1, 0, 0] and list(t.live) == [True, True, True, False]


def test_forward_outcomes(small):
    out, listed = total(small, "outcomes"), total(small, "listed_outcomes")
    print("forward census outcomes", dict(zip(("local", "delivered", "unreachable", "hop_limit", "no_owner", "entry_down"),
                                              out.tolist())), "listed", listed.tolist())
    for code in (FC.LOCAL, FC.DELIVERED, FC.UNREACHABLE, FC.HOP_LIMIT, FC.NO_OWNER):
        assert out[code] > 0, code
    assert out[FC.ENTRY_DOWN] == 0, "the census enters at live rows only"
    assert listed[FC.ENTRY_DOWN] > 0, "dead rows are entries of the listed call"
    print("split keys", total(small, "split_keys"), "most at one checkpoint", max(r["split_keys_max"] for r in small.values()))
    assert total(small, "split_keys") >= 1


def test_server_count_classes(small):
    classes = {k: sum(r["servers"][k] for r in small.values()) for k in ("empty", "1-3", "4-16", ">16")}
    print("checkpoints", total(small, "checkpoints"), "rows", total(small, "rows"), "of dead observers",
          total(small, "dead_rows"), "views by server count", classes)
    assert all(v > 0 for v in classes.values()), classes
    assert total(small, "dead_rows") > 0


@pytest.mark.slow
def test_distinct_views_at_257(large):
    most = {k: r["distinct_views_max"] for k, r in large.items()}
    print("distinct views at 257 members", most)
    assert max(most.values()) >= 257 - 1


def test_census_columns_and_incarnations(small):
    cells = total(small, "cells")
    print("census cells", cells.tolist(), "min != max", total(small, "min_max_differ"), "largest spread in periods",
          max(r["incarnation_spread_max"] for r in small.values()))
    assert (cells > 0).all(), cells
    assert total(small, "min_max_differ") > 0
    for (n, seed), r in small.items():
        assert (r["cells"] > 0).all(), f"case {n}-{seed} reaches every cell value: {r['cells']}"


def test_disagreement(small):
    print("distinct ring checksums among live rows, most", max(r["ring_checksums_live_max"] for r in small.values()),
          "disagreeing keys", total(small, "disagreeing_keys"), "most at one checkpoint",
          max(r["disagreeing_keys_max"] for r in small.values()), "replica sets", total(small, "replica_disagreeing_keys"))
    assert max(r["ring_checksums_live_max"] for r in small.values()) >= 2
    assert total(small, "disagreeing_keys") >= 1
    assert total(small, "replica_disagreeing_keys") >= 1


@pytest.mark.slow
def test_checkpoints_at_1100():
    """what tests/test_fuzz_views.py checks at 1,100 members, on the oracle: the two checkpoints exist, the tracker's
    liveness is the oracle's after every call, the sample holds the observers it is meant to hold, and the chains of the
    sampled entries stay inside the rows whose owners were computed"""
    c = F.mass_case(1100, 0)
    n = c["n"]
    ora = OracleSim(n, init=c["init"], **c["options"])
    tracker = V.Tracker(n)
    last = len(c["calls"]) - 1
    mid = next(i for i, call in enumerate(c["calls"]) if call["round"] <= 8 < call["round"] + call["rounds"])
    assert F.MASS_CUT_ROUND <= 8 < F.MASS_JOIN_ROUND and mid < last
    for i, call in enumerate(c["calls"]):
        F.oracle_call(ora, call)
        tracker.apply(call)
        assert [ora.live(o) for o in range(n)] == list(tracker.live), f"liveness after call {i}"
        if i not in (mid, last):
            continue
        view = V.RowsView(ora.rows(), tracker.live)
        sample = V.sampled_observers(c, tracker)
        assert len(sample) == len(set(sample)) == V.SAMPLED and sample[:2] == [0, n - 1]
        assert not all(tracker.live[sample])
        owners, known = V.owners_closure(view, V.KEYS16, 100, sample, V.HOPS[0])
        want = FC.chase_grid(owners, tracker.live, tracker.part, sample, V.HOPS[0])
        assert known[want[3]].all() and (want[4] >= -1).all()
        outcomes = np.bincount(want[0].ravel(), minlength=6)
        views = len({r.tobytes() for r in view.rows()[0] <= 1})
        print(f"call {i}: {int((~tracker.live).sum())} dead, labels {np.bincount(tracker.part).tolist()}, {views} distinct "
              f"views, {int(known.sum())} rows in the closure, sampled outcomes {outcomes.tolist()}")
        assert outcomes[FC.ENTRY_DOWN] > 0 and outcomes[FC.DELIVERED] > 0
        if i == mid:
            assert (tracker.part[sample] == 1).any() and (tracker.part == 1).sum() >= n // 3
            assert outcomes[FC.UNREACHABLE] > 0 and views > 500
