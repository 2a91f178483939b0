"""The read-only view calls of the MI355X engine on the states of the seeded random schedules, against the CPU oracle.

Every committed case of at least 5 members runs as tests/test_fuzz.py runs it (run_case: all of its comparisons stay
on), and from its after_call hook tests/fuzz_views.py check_views compares census, route / route_census (R = 100 with 64
keys, R = 1 with 9), route_n / replica_census (n = 3 and 16), ring_checksums / ring_census and forward / forward_census
(8 hops and 1, chain and one_hop, every row an entry) in every mode with the restatements the hand-written scenarios
use, exactly, for every row and key: after every call up to 130 members, after the first call, every fourth after it
and the last at 257. The run's own comparisons after those calls are what test that a view call changes no state and no
result of a round, on states with pending dissemination, fired timers, hot columns and deferred decisions in them.

Every run also traces min(n, 64) members (every ceil(n / 64)-th) from before round 0: the trace is drained after each
call and compared record for record with expected(ora, "live", members) and the live count taken after each of the
oracle's rounds, over the schedule's chunked calls with events and raw mutators between them.

tests/test_fuzz_views_host.py asserts, on the oracle alone, what these checkpoints hold.

First run on MI355X: all 38 tests passed; no divergence. Durations there: 0.9 to 1.4 s per case at 5 members, 2.7 to
4.1 s at 63 to 65, 1.8 to 9.2 s at 127 to 130 and 5.8 to 13.1 s at 257; the sharded runs 3.7 to 11.9 s, the variants 3.0
to 6.0 s, the 1,100-member runs 5.5 s (one handle) and 0.9 s (three shards, after it); the file 203 s. The oracle ring's
answers are kept per view for the session (test_route.answers_of): without that the file took 251 s.
"""
import time

import numpy as np
import pytest

import fuzz_scenarios as F
import fuzz_views as V
import swimsim
import test_census as TC
import test_fuzz_at_size as TS
from oracle_ffi import OracleSim
from test_engine_parity import make_pair
from test_fuzz import run_case

pytestmark = pytest.mark.gpu

REFUSAL = "EINVAL.*chains that cross shards"


def run_with_views(eng, ora, c, label, forward=True):
    """run_case with the member trace compared after every call and check_views at the case's checkpoints; returns
    what the checkpoints held (fuzz_views.new_reach)"""
    n = c["n"]
    tracker = V.Tracker(n)
    members = V.traced_members(n)
    checked = V.checkpoint_calls(c)
    reach = V.new_reach()
    pending, at = [], [0]
    eng.trace_members(members, 64)

    def after_round(r):
        pending.append((r, sum(ora.live(o) for o in range(n)), TC.expected(ora, "live", members)[0]))

    def after_call():
        i, at[0] = at[0], at[0] + 1
        call = c["calls"][i]
        where = f"{label} after round {call['round'] + call['rounds'] - 1}"
        tracker.apply(call)
        rounds, nlive, counts, dropped = eng.trace()
        assert dropped == 0 and list(rounds) == [p[0] for p in pending] == list(range(call["round"], call["round"] + call["rounds"]))
        assert list(nlive) == [p[1] for p in pending], f"{where}: trace live counts {list(nlive)} oracle {[p[1] for p in pending]}"
        for k, (r, _, want) in enumerate(pending):
            bad = np.argwhere(counts[k] != want)
            assert not len(bad), (f"{where}: trace of round {r}, member {members[bad[0][0]]}: engine {counts[k][bad[0][0]]} "
                                  f"oracle {want[bad[0][0]]}\n{F.describe_call(call)}")
        pending.clear()
        if i in checked:
            V.check_views(eng, ora, tracker.part, V.KEYS64, R=100, what=where, forward=forward, reach=reach)
            if not forward:
                with pytest.raises(swimsim.SwimsimError, match=REFUSAL):
                    eng.forward(V.KEYS64, [0])
                with pytest.raises(swimsim.SwimsimError, match=REFUSAL):
                    eng.forward_census(V.KEYS64)

    run_case(eng, ora, c, label, after_call, after_round)
    assert at[0] == len(c["calls"]) and reach["checkpoints"] == len(checked)
    return reach


@pytest.mark.parametrize("n,seed", V.CASES, ids=[f"{n}-{s}" for n, s in V.CASES])
def test_views_on_random_schedule(n, seed):
    c = F.case(n, seed)
    eng, ora = make_pair(n, init=c["init"], **c["options"])
    try:
        reach = run_with_views(eng, ora, c, f"case {n}-{seed}")
        print(f"case {n}-{seed}: {reach}")
    finally:
        eng.close()


@pytest.mark.parametrize("n,seed", F.VARIANT_CASES, ids=[f"{n}-{s}" for n, s in F.VARIANT_CASES])
@pytest.mark.parametrize("shards", [2, 3])
def test_views_on_random_schedule_sharded(shards, n, seed):
    """over 2 and 3 shards (65 rows over 3 is uneven), direct heals as events: everything but the forward calls, which a
    sharded cluster refuses with the documented EINVAL text"""
    c = F.without_direct_heal(F.case(n, seed))
    eng = swimsim.ShardedCluster(n, shards, init=c["init"], **c["options"])
    try:
        ora = OracleSim(n, init=c["init"], **c["options"])
        run_with_views(eng, ora, c, f"case {shards}-{n}-{seed}", forward=False)
    finally:
        eng.close()


VARIANTS = {"cs_defer2": {"cs_defer": 2}, "hot_slots0": {"hot_slots": 0}}


@pytest.mark.parametrize("n,seed", [(65, 1), (130, 0)], ids=["65-1", "130-0"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_views_on_random_schedule_variants(variant, n, seed):
    """cs_defer = 2 leaves rows unhashed inside a call, and the trace kernel runs after phase C; hot_slots = 0 keeps
    every member on the dense path"""
    c = F.case(n, seed)
    eng, ora = make_pair(n, init=c["init"], tuning=VARIANTS[variant], **c["options"])
    try:
        run_with_views(eng, ora, c, f"case {variant}-{n}-{seed}")
        units = eng.kernel_units()
        assert variant != "cs_defer2" or units["cs_skipped_rounds"] > 0
        assert variant != "hot_slots0" or units["hot_slots"] == 0
    finally:
        eng.close()


# ---- at 1,100 members ------------------------------------------------------------------------------------------------

def at_size(eng, c, want, label, forward):
    """run_against_records with check_views_at_size after the call that holds round 8 and after the last call"""
    tracker = V.Tracker(c["n"])
    at, spent = [0], []
    last = len(c["calls"]) - 1
    mid = next(i for i, call in enumerate(c["calls"]) if call["round"] <= 8 < call["round"] + call["rounds"])
    assert mid < last

    def after_call():
        i, at[0] = at[0], at[0] + 1
        call = c["calls"][i]
        tracker.apply(call)
        if i not in (mid, last):
            return
        t0 = time.time()
        view = V.RowsView(eng.rows(), tracker.live)
        sample = V.sampled_observers(c, tracker)
        assert len(sample) == V.SAMPLED and not all(tracker.live[sample])
        V.check_views_at_size(eng, view, tracker.part, sample, forward=forward,
                              what=f"{label} after round {call['round'] + call['rounds'] - 1}")
        if not forward:
            with pytest.raises(swimsim.SwimsimError, match=REFUSAL):
                eng.forward_census(V.KEYS16)
        spent.append(round(time.time() - t0, 2))
        if i == mid:
            assert tracker.part.any() and not tracker.live.all(), "the cut is in force and killed members are down"

    TS.run_against_records(eng, c, want, label, after_call)
    assert len(spent) == 2
    print(f"{label}: seconds in the two view checkpoints {spent}")


def test_views_at_1100():
    """Case 1100-0 against its committed records, with the view calls after the call that contains round 8 (the cut is in
    force and the killed members are turning faulty) and after the last call. At those points the per-call record has
    just proved the engine's rows equal to the oracle's, so the expected values are computed on the host from eng.rows(),
    the schedule's liveness and partition labels (fuzz_views.Tracker) through the same oracle rings and restatements.
    The code under test (the route, ring-checksum, census and forward kernels) is not the code that produced the rows:
    rows() is a copy of the state the round kernels wrote. All rows: the census, the ring checksums and their census, and
    route / route_census, route_n / replica_census (n = 3) and forward / forward_census at R = 2 with 16 keys. 48 sampled
    observers (0, 1,099, a killed member, a member of the cut among them): route, route_n (n = 16) and the listed
    forward at R = 100 with the same 16 keys, the forward over the owners of every row its chains can visit."""
    c = F.mass_case(1100, 0)
    eng = swimsim.Cluster(1100, init=c["init"], **c["options"])
    try:
        at_size(eng, c, TS.load_fixture(1100, 0), "case views-1100-0", True)
    finally:
        eng.close()


def test_views_at_1100_sharded():
    """the same over 3 shards (367, 367 and 366 rows): everything but the forward calls, which are refused"""
    c = F.mass_case(1100, 0)
    cs = F.without_direct_heal(c)
    fx = TS.load_fixture(1100, 0)
    eng = swimsim.ShardedCluster(1100, 3, init=cs["init"], **cs["options"])
    try:
        at_size(eng, cs, fx if fx["sharded"] == "same" else fx["sharded"], "case views-3-1100-0", False)
    finally:
        eng.close()
