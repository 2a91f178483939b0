"""The mass fuzz schedules (tests/fuzz_scenarios.py mass_case) on the CPU oracle alone: the generator is deterministic
and stays inside the input bounds, the committed records (tests/golden/fuzz_mass_*.json, written by
tests/golden/make_fuzz_fixtures.py on the OpenMP oracle) are what the single-threaded oracle gives, and every case
reaches what it was written to reach, whatever the engine does. The reach conditions are conditions on the input, read
from each fixture's "reach" block."""
import collections
import json
import os

import pytest

import fuzz_records as R
import fuzz_scenarios as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHARDED = ((1100, 0), (2304, 0))
IDS = [f"{n}-{s}" for n, s in F.MASS_CASES]


def load_fixture(n, seed):
    path = os.path.join(GOLDEN, f"fuzz_mass_n{n}_s{seed}.json")
    if not os.path.exists(path):
        pytest.fail(f"missing fixture {os.path.basename(path)}: run tests/golden/make_fuzz_fixtures.py")
    with open(path) as f:
        return json.load(f)


def test_mass_case_is_deterministic():
    assert F.MASS_ROUNDS == 30 and F.MASS_CASES == [(1100, 0), (2304, 0), (4160, 0), (4160, 1)]
    for n, seed in F.MASS_CASES:
        assert F.mass_case(n, seed) == F.mass_case(n, seed)
    assert F.mass_case(4160, 0) != F.mass_case(4160, 1)


def test_mass_schedules_stay_inside_the_input_bounds():
    for n, seed in F.MASS_CASES:
        c = F.mass_case(n, seed)
        base = F.case(n, seed, F.MASS_ROUNDS)
        assert c["init"] == "converged" and c["options"] == base["options"] and c["watch"] == base["watch"]
        assert sum(call["rounds"] for call in c["calls"]) == c["rounds"] == F.MASS_ROUNDS
        assert not c["calls"][0]["muts"]
        at = 0
        for call, bcall in zip(c["calls"], base["calls"]):
            assert call["round"] == at and (call["rounds"] in (1, 2, 3, 7) or at + call["rounds"] == F.MASS_ROUNDS)
            at += call["rounds"]
            assert call["muts"] == bcall["muts"] and (call["round"], call["rounds"]) == (bcall["round"], bcall["rounds"])
            per_round = collections.Counter(e[0] for e in call["events"])
            assert all(call["round"] <= r < at for r in per_round) and max(per_round.values(), default=0) <= 4 * n + 64
            assert [e[0] for e in call["events"]] == sorted(e[0] for e in call["events"])
            for r in range(call["round"], at):                     # a round's base events come first, in their order
                mine, theirs = [e for e in call["events"] if e[0] == r], [e for e in bcall["events"] if e[0] == r]
                assert mine[:len(theirs)] == theirs
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
        assert len(c["calls"]) == len(base["calls"])
        assert len(load_fixture(n, seed)["calls"]) == len(c["calls"])


def test_mass_events_take_a_fraction_of_the_cluster():
    for n, seed in F.MASS_CASES:
        ev = [e for call in F.mass_case(n, seed)["calls"] for e in call["events"]]
        at = lambda r, k, b=0: {a for (rr, kk, a, bb) in ev if (rr, kk, bb) == (r, k, b)}
        assert len(at(F.MASS_REINCARNATE_ROUND, F.EV_REINCARNATE)) >= int(F.MASS_REINCARNATE_FRACTION * n)
        killed = at(F.MASS_KILL_ROUND, F.EV_KILL)
        assert len(killed) >= max(2, n // 32)
        cut = at(F.MASS_CUT_ROUND, F.EV_PARTITION, 1)
        assert len(cut) >= n // 3 and at(F.MASS_JOIN_ROUND, F.EV_PARTITION, 0) >= cut
        assert at(F.MASS_HEAL_ROUND, F.EV_HEAL) & cut
        assert len(at(F.MASS_REVIVE_ROUND, F.EV_REVIVE) & killed) >= len(killed) // 2
        assert len(at(F.MASS_REAP_ROUND, F.EV_REAP)) >= 3
        assert sum(1 for e in ev if e[1] == F.EV_LEAVE) >= 4


def check_against_oracle(n, seed):
    """the committed records of case (n, seed) are the single-threaded oracle's"""
    fx = load_fixture(n, seed)
    c = F.mass_case(n, seed)
    _, out, _ = R.oracle_records(c)
    for i, (got, want) in enumerate(zip(out["calls"], fx["calls"])):
        call = c["calls"][i]
        assert got == want, (f"case {n}-{seed}: call {i} differs from the fixture: {got} against {want}\n"
                             f"{F.describe_call(dict(call, events=call['events'][:40]))} ...")
    assert out["final"] == fx["final"]
    assert ("sharded" in fx) == ((n, seed) in SHARDED)
    if (n, seed) in SHARDED:
        cs = F.without_direct_heal(c)
        if cs == c:
            assert fx["sharded"] == "same"
        else:
            assert R.oracle_records(cs)[1] == fx["sharded"]


def test_fixture_1100_is_the_single_threaded_oracles():
    check_against_oracle(1100, 0)


@pytest.mark.slow
@pytest.mark.parametrize("n,seed", F.MASS_CASES[1:], ids=IDS[1:])
def test_larger_fixtures_are_the_single_threaded_oracles(n, seed):
    check_against_oracle(n, seed)


# ---- reach: what each committed case did on the oracle ----
@pytest.mark.parametrize("n,seed", F.MASS_CASES, ids=IDS)
def test_reach_of_each_case(n, seed):
    reach = load_fixture(n, seed)["reach"]
    print(f"{n}-{seed}: {reach}")
    assert reach["evicted"] > 0
    for k in ("timers_fired", "pingreqs", "helper_errors", "refutes", "heal_attempts", "suspect_decl"):
        assert reach["counters"][k] > 0, k
    assert reach["row_changes_max"] > 1024                         # past the undo log of one receive phase's row
    if n > 4096:
        assert reach["row_changes_max"] > 2048                     # past the hot columns
        assert reach["evicted_member_max"] >= 4096 and reach["evicting_observer_max"] >= 4096   # the 65th timer block


def test_reach_over_all_cases():
    reaches = [load_fixture(n, seed)["reach"] for n, seed in F.MASS_CASES]
    assert any(r["counters"]["full_syncs"] > 0 for r in reaches)
    for name in F.EVENT_NAMES.values():
        assert sum(r["events"].get(name, 0) for r in reaches) >= 1, name
    for name in F.MUTATORS:
        assert sum(r["mutators"].get(name, 0) for r in reaches) >= 1, name


def test_reach_block_counts_the_schedule():
    """the event and mutator counts of the reach blocks are those of the schedules as generated now"""
    for n, seed in F.MASS_CASES:
        c, reach = F.mass_case(n, seed), load_fixture(n, seed)["reach"]
        assert reach["events"] == dict(collections.Counter(F.EVENT_NAMES[e[1]] for call in c["calls"]
                                                           for e in call["events"]))
        assert reach["mutators"] == dict(collections.Counter(m[0] for call in c["calls"] for m in call["muts"]))


def test_fixtures_stay_small():
    for n, seed in F.MASS_CASES:
        assert os.path.getsize(os.path.join(GOLDEN, f"fuzz_mass_n{n}_s{seed}.json")) < 121_553
