"""The mass fuzz schedules (tests/fuzz_scenarios.py mass_case: all eight event kinds, the raw mutators, short timeouts,
a 30-period clock step, chunked step calls, with a fraction of the cluster taking part) on the MI355X engine at 1,100,
2,304 and 4,160 members, against the committed records of the CPU oracle (tests/golden/fuzz_mass_*.json, written by
tests/golden/make_fuzz_fixtures.py; tests/test_fuzz_at_size_host.py pins them to the single-threaded oracle and
asserts what the schedules reach there).

The engine runs each schedule as tests/test_fuzz.py does: the mutators, then the chunked step. After every call its
record (tests/fuzz_records.py call_record) is compared with the fixture's field by field, after the last call the final
record. Everything is integer work: the bar is bit-exact. On the first mismatch the schedule is replayed on the live
single-threaded oracle up to that call (slow, and only then), and the failure names the first differing row, buffer,
timer or counter and lists the call's events and mutators.

Engine-side traces of the production runs: the largest value of seven kernel_units() counters after any call, printed per
case. Measured on MI355X at the first run (the assertions in PRODUCTION_TRACES are what that run showed):

  case     hot_slots  lazy_late  dense_resp  dense_jobs  defer_undo_over  cs_rows_narrow  cs_rows_wide
  1100-0       1,091          0           0           0                0          25,375             0
  2304-0       2,048         63           2           2                0          62,623             0
  4160-0       2,048      5,179           0           0                0         105,249             0
  4160-1       2,048      3,025           0           0                0         109,000             0

Traces that stayed at zero, and are therefore not asserted:
  * defer_undo_over in every case and variant, although an observer changes up to 4,149 cells in one round on the
    oracle. Rows whose receive-phase undo log passes its capacity do occur: they are counted by lazy_late (a pending
    sender's wave rebuilds its issue-time row when its log runs over, k_recv), at 2,304 and 4,160 members, not at 1,100.
  * cs_rows_wide on the production engine: no phase-C launch of these runs is wide. The cs_ref variant counts 4,384
    rows there and 15,921 narrow ones, with delta launches > 0.
  * dense_resp and dense_jobs at 1,100 and 4,160 members (2 each at 2,304, the one case with full syncs: 2 on the oracle).
The variants on (2304, 0) measured: hot_slots 0 under hot_slots0; side_cap 0 under cs_async0; lazy_late 26,406 under
defer_test8 (63 in production).
"""
import collections
import functools
import json
import os
import time

import pytest

import fuzz_records as R
import fuzz_scenarios as F
import swimsim
from test_engine_parity import full_diff

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRACES = ("hot_slots", "defer_undo_over", "lazy_late", "dense_resp", "dense_jobs", "cs_rows_narrow", "cs_rows_wide")
IDS = [f"{n}-{s}" for n, s in F.MASS_CASES]


@functools.lru_cache(maxsize=None)
def load_fixture(n, seed):
    path = os.path.join(GOLDEN, f"fuzz_mass_n{n}_s{seed}.json")
    if not os.path.exists(path):
        pytest.fail(f"missing fixture {os.path.basename(path)}: run tests/golden/make_fuzz_fixtures.py")
    with open(path) as f:
        return json.load(f)


def describe(call, most=40):
    """describe_call of a call with thousands of events: its mutators, the events counted by (round, kind), the first"""
    if len(call["events"]) <= most:
        return F.describe_call(call)
    counts = collections.Counter((r, F.EVENT_NAMES[k]) for (r, k, a, b) in call["events"])
    return (f"{len(call['events'])} events, by round and kind {dict(counts)}; the first {most}: "
            f"{F.describe_call(dict(call, events=call['events'][:most]))}")


def mismatch(eng, c, i, what):
    """fail with the first differing state: the schedule on the live oracle up to call i, against the engine as it is"""
    ora, _, _ = R.oracle_records(c, upto=i)
    call = c["calls"][i]
    pytest.fail(f"after round {call['round'] + call['rounds'] - 1} (call {i}): {what}: "
                f"{full_diff(eng, ora, c['n'])}\n{describe(call)}")


def run_against_records(eng, c, want, label, after_call=None):
    """the schedule on the engine, every call's record and the final record against the oracle's (want); returns the
    seconds spent in the mutators and step calls, in the calls' records and in the final record"""
    try:
        return _run_against_records(eng, c, want, label, after_call)
    except swimsim.SwimsimError as e:
        if "EHIP" in str(e):                                        # a device error: nothing more runs on this GPU
            pytest.exit(f"{label}: device error, the session ends here: {e}", returncode=3)
        raise


def _run_against_records(eng, c, want, label, after_call):
    assert len(want["calls"]) == len(c["calls"])
    R.start_watching(eng, c)
    spent = [0.0, 0.0, 0.0]
    for i, (call, rec) in enumerate(zip(c["calls"], want["calls"])):
        t0 = time.time()
        try:
            rets = [x for m, x in ((m, F.apply_mutator(eng, m)) for m in call["muts"]) if m[0] in F.COMPARED_RETURNS]
            eng.step(call["rounds"], call["events"])
            eng.digest()                                            # (the step call's work has ended)
        except swimsim.SwimsimError as e:
            if "EHIP" in str(e):
                raise
            pytest.fail(f"{label}: the engine refused: {e}\n{describe(call)}")
        t1 = time.time()
        got = R.call_record(eng, c, call, rets)
        spent[0] += t1 - t0
        spent[1] += time.time() - t1
        assert got.keys() == rec.keys()
        for k in rec:
            if got[k] != rec[k]:
                mismatch(eng, c, i, f"{label}: {k} differs: engine {got[k]} oracle {rec[k]}")
        if after_call:
            after_call()
    assert eng.round == c["rounds"]
    t0 = time.time()
    got = R.final_record(eng, c)
    spent[2] = time.time() - t0
    assert got.keys() == want["final"].keys()
    for k in want["final"]:
        if got[k] != want["final"][k]:
            mismatch(eng, c, len(c["calls"]) - 1, f"{label}: final {k} differs")
    return [round(x, 2) for x in spent]


def run_engine(n, seed, tuning, label):
    """case (n, seed) on one Cluster under a tuning block against the fixture; returns the largest value of each trace
    counter after any call (hot_slots drops to 0 at a raw write), kernel_units(), memory(), checksum_path_stats()"""
    c = F.mass_case(n, seed)
    peak = dict.fromkeys(TRACES, 0)
    eng = swimsim.Cluster(n, init=c["init"], tuning=tuning, **c["options"])

    def after_call():
        u = eng.kernel_units()
        for k in TRACES:
            peak[k] = max(peak[k], int(u[k]))

    try:
        spent = run_against_records(eng, c, load_fixture(n, seed), label, after_call)
        print(f"{label}: seconds in steps, call records, final record {spent}, traces {peak}")
        return peak, eng.kernel_units(), eng.memory(), eng.checksum_path_stats()
    finally:
        eng.close()


# what the production engine's first run on MI355X showed, per case (the module docstring has every measured value)
PRODUCTION_TRACES = {
    (1100, 0): lambda p: p["hot_slots"] > 1024,                    # more than one slot per thread of a 1,024-thread pass
    (2304, 0): lambda p: p["hot_slots"] == 2048 and p["lazy_late"] > 0 and p["dense_resp"] > 0 and p["dense_jobs"] > 0,
    (4160, 0): lambda p: p["hot_slots"] == 2048 and p["lazy_late"] > 0,
    (4160, 1): lambda p: p["hot_slots"] == 2048 and p["lazy_late"] > 0,
}


@pytest.mark.parametrize("n,seed", F.MASS_CASES, ids=IDS)
def test_mass_schedule(n, seed):
    peak, units, mem, paths = run_engine(n, seed, None, f"case {n}-{seed}")
    print(f"case {n}-{seed}: units { {k: v for k, v in units.items() if v} } memory {mem} checksum paths {paths}")
    assert peak["cs_rows_narrow"] > 0 and PRODUCTION_TRACES[(n, seed)](peak), f"case {n}-{seed}: traces {peak}"


# ---- tuning variants on (2304, 0): the same records, and a trace that the variant's path ran ----
VARIANTS = {
    # the reference-row checksum path over rows that hold evicted, tombstoned and left members. cs_async = 0 because a
    # side-stream launch takes that path only from 4,097 rows on (csr_side_wanted): with the side stream on, no launch of
    # a 2,304-row cluster reaches it (measured: delta_launches 0 under {"cs_ref": 2, "cs_narrow_rows": 0} alone)
    "cs_ref": ({"cs_ref": 2, "cs_async": 0, "cs_narrow_rows": 0},
               lambda p, u, m, s: u["cs_rows_wide"] > 0 and s["delta_launches"] > 0),
    "hot_slots0": ({"hot_slots": 0}, lambda p, u, m, s: p["hot_slots"] == 0),
    "cs_async0": ({"cs_async": 0}, lambda p, u, m, s: m["side_cap"] == 0),
    "defer_test8": ({"defer_test": 8}, lambda p, u, m, s: u["lazy_late"] > 0),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_mass_schedule_variants(variant):
    tuning, trace = VARIANTS[variant]
    run = run_engine(2304, 0, tuning, f"case {variant}-2304-0")
    print(f"{variant}: units { {k: v for k, v in run[1].items() if v} } memory {run[2]} checksum paths {run[3]}")
    assert trace(*run), f"{variant} left no trace in this run: {run}"


@pytest.mark.parametrize("shards,n,seed", [(3, 1100, 0), (2, 2304, 0)], ids=["3-1100-0", "2-2304-0"])
def test_mass_schedule_sharded(shards, n, seed):
    """over 3 shards (367, 367 and 366 rows) and over 2; a sharded cluster refuses the direct heal call, so those heals
    run as events, and the records are those of that case"""
    c = F.mass_case(n, seed)
    cs = F.without_direct_heal(c)
    fx = load_fixture(n, seed)
    want = fx if fx["sharded"] == "same" else fx["sharded"]
    assert (fx["sharded"] == "same") == (cs == c)
    eng = swimsim.ShardedCluster(n, shards, init=cs["init"], **cs["options"])
    try:
        spent = run_against_records(eng, cs, want, f"case {shards}-{n}-{seed}")
        print(f"case {shards}-{n}-{seed}: seconds in steps, call records, final record {spent}")
    finally:
        eng.close()
