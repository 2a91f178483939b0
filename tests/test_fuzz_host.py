"""The fuzz schedules (tests/fuzz_scenarios.py) on the CPU oracle alone: the generator is deterministic, and the
committed case list reaches what it was written to reach, whatever the engine does. The replay is the one
tests/test_fuzz.py runs on the oracle side (fuzz_scenarios.oracle_call)."""
import collections

import pytest

import fuzz_scenarios as F
from oracle_ffi import COUNTER_NAMES, UNKNOWN, OracleSim


def test_case_is_deterministic():
    for n, seed in ((1, 0), (3, 2), (65, 1), (257, 0)):
        assert F.case(n, seed) == F.case(n, seed)
    assert F.case(65, 0) != F.case(65, 1)
    assert F.case(64, 0)["calls"] != F.case(65, 0)["calls"]


def test_schedules_stay_inside_the_input_bounds():
    for n, seed in F.CASES:
        c = F.case(n, seed)
        assert sum(call["rounds"] for call in c["calls"]) == c["rounds"] == 60
        assert not c["calls"][0]["muts"]
        at = 0
        for call in c["calls"]:
            assert call["round"] == at and (call["rounds"] in (1, 2, 3, 7) or at + call["rounds"] == 60)
            at += call["rounds"]
            per_round = collections.Counter(e[0] for e in call["events"])
            assert all(call["round"] <= r < at for r in per_round) and max(per_round.values(), default=0) <= 4 * n + 64
            for (r, k, a, b) in call["events"]:
                assert 0 <= a < n and (k != F.EV_CLOCK or (r + b >= 0 and abs(b) <= 30))
                assert k != F.EV_PARTITION or b in (0, 1, 2)
            for m in call["muts"]:
                if m[0] == "set_member":
                    assert m[1] != m[2]
                if m[0] == "set_clock_offset":
                    assert call["round"] + m[2] >= 0
                if m[0] == "add_join_list":
                    assert len(set(m[2])) == len(m[2])
        assert c["options"]["ping_request_size"] <= 8 and c["options"]["p_factor"] * 3 <= 255


def test_oracle_clock_event_runs_in_list_order():
    """OR_EV_CLOCK (docs/ROUND_SEMANTICS.md §4 E): offset_a = b periods, in list order. A reincarnate before it takes the
    old clock, one after it the new one; the round equals one with set_clock_offset called before it."""
    P, T0 = F.PERIOD_MS, F.T0_MS
    a, b = OracleSim(8), OracleSim(8)
    for s in (a, b):
        s.run(4)
    a.step([(4, F.EV_REINCARNATE, 2, 0), (4, F.EV_CLOCK, 2, 5), (4, F.EV_CLOCK, 3, -2), (4, F.EV_REINCARNATE, 3, 0)])
    assert a.member(2, 2) == (0, T0 + 4 * P) and a.member(3, 3) == (0, T0 + 2 * P)
    assert list(a.clock_offsets()) == [0, 0, 5 * P, -2 * P, 0, 0, 0, 0]
    b.set_clock_offset(3, -2 * P)
    b.step([(4, F.EV_REINCARNATE, 2, 0), (4, F.EV_REINCARNATE, 3, 0)])
    b.set_clock_offset(2, 5 * P)
    assert a.digest() == b.digest() and (a.checksums() == b.checksums()).all()
    a.step([(5, F.EV_REINCARNATE, 2, 0)])
    assert a.member(2, 2) == (0, T0 + 10 * P)


@pytest.fixture(scope="module")
def coverage():
    """every committed case on the oracle, once: what the runs reached, summed"""
    cov = {"counters": collections.Counter(), "events": collections.Counter(), "mutators": collections.Counter(),
           "multi": 0, "evicted": 0, "make_change": collections.Counter(), "big_jumps": 0}
    for n, seed in F.CASES:
        c = F.case(n, seed)
        ora = OracleSim(n, init=c["init"], **c["options"])
        for o in c["watch"]:
            ora.watch(o, "events")
        rows = {}

        def before_round(r):
            rows["st"] = ora.rows()[0]

        def after_round(r):
            # (mutators run between rounds: a cell that turns UNKNOWN inside a round was evicted by a timer)
            cov["evicted"] += int(((rows["st"] != UNKNOWN) & (ora.rows()[0] == UNKNOWN)).sum())

        for call in c["calls"]:
            for m in call["muts"]:
                cov["mutators"][m[0]] += 1
            mc = [m for m in call["muts"] if m[0] in F.COMPARED_RETURNS]
            rets = F.oracle_call(ora, call, before_round, after_round)
            for m, x in zip(mc, rets):
                if m[0] == "make_change":
                    cov["make_change"][x] += 1
            for (r, k, a, b) in call["events"]:
                cov["events"][k] += 1
                cov["big_jumps"] += k == F.EV_CLOCK and abs(b) == 30
            pairs = collections.Counter((r, a) for (r, k, a, b) in call["events"])
            cov["multi"] += sum(1 for v in pairs.values() if v >= 2)
        assert ora.round == c["rounds"]
        for k, v in ora.counters().items():
            cov["counters"][k] += v
    return cov


def test_every_oracle_counter_is_reached(coverage):
    print({k: coverage["counters"][k] for k in COUNTER_NAMES})
    assert len(COUNTER_NAMES) == 18
    zero = [k for k in COUNTER_NAMES if coverage["counters"][k] == 0]
    assert not zero, f"counters never reached: {zero}"


def test_every_event_kind_and_mutator_occurs_20_times(coverage):
    print(dict(coverage["events"]), dict(coverage["mutators"]))
    for k, name in F.EVENT_NAMES.items():
        assert coverage["events"][k] >= 20, name
    for name in F.MUTATORS:
        assert coverage["mutators"][name] >= 20, name
    assert coverage["big_jumps"] == len(F.CASES)


def test_members_with_several_events_in_one_round(coverage):
    assert coverage["multi"] >= 10, coverage["multi"]


def test_make_change_returns_both_values(coverage):
    assert coverage["make_change"][0] >= 1 and coverage["make_change"][1] >= 1, dict(coverage["make_change"])


def test_a_cell_is_evicted(coverage):
    print(coverage["evicted"], "cells evicted")
    assert coverage["evicted"] >= 1
