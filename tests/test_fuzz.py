"""Seeded random schedules on the MI355X engine against the CPU oracle (tests/fuzz_scenarios.py has the generator and its
restrictions, tests/test_fuzz_host.py what the committed cases reach on the oracle alone).

The engine runs each schedule in its chunked step calls, with the raw mutators between the calls; the oracle steps round
by round. After every call the checksums, the three state digests, the last ping targets, the counters and converged()
are compared, with the return value of every make_change and add_join_list and the target list of every direct heal,
and the per-Update event streams of two watched observers. After the last call every observer's row, dissemination
buffer, timers, iterator, node statistics and clock offset are compared. Everything is integer work: the bar is
bit-exact. A failure names the case, the round and the first differing state, and lists the last call's events and
mutators; the parametrize id alone reproduces it (case(n, seed) is deterministic).
"""
import functools

import numpy as np
import pytest

import fuzz_scenarios as F
import swimsim
from oracle_ffi import OracleSim
from test_engine_parity import full_diff, make_pair

pytestmark = pytest.mark.gpu


def compare_call(eng, ora, c, call, label, erets, orets):
    n = c["n"]
    where = f"{label} after round {call['round'] + call['rounds'] - 1}"

    def fail(what):
        pytest.fail(f"{where}: {what}: {full_diff(eng, ora, n)}\n{F.describe_call(call)}")

    if erets != orets:
        fail(f"mutator results differ: engine {erets} oracle {orets}")
    ec, oc = eng.checksums(), ora.checksums()
    if not (ec == oc).all():
        fail(f"checksums differ at observers {np.nonzero(ec != oc)[0][:5]}")
    if eng.digest() != ora.digest():
        fail(f"digests differ: engine {eng.digest()} oracle {ora.digest()}")
    et, ot = eng.last_targets(), ora.last_targets()
    if not (et == ot).all():
        fail(f"targets differ at observers {np.nonzero(et != ot)[0][:5]}")
    if eng.counters() != ora.counters():
        fail("counters differ")
    if eng.converged() != ora.converged():
        fail(f"converged: engine {eng.converged()} oracle {ora.converged()}")
    for o in c["watch"]:
        ee, eold, enew, enm = eng.applied_events(o)
        oe, oold, onew, onm = ora.drain_events(o)
        oe = [sorted(x) for x in oe]                                # (one Update's changes: member order)
        if ee != oe:
            i = next((i for i, (a, b) in enumerate(zip(ee, oe)) if a != b), min(len(ee), len(oe)))
            fail(f"event stream of {o}: {len(ee)} events on the engine, {len(oe)} in the oracle, first difference at "
                 f"{i}: {ee[i:i + 1]} vs {oe[i:i + 1]}")
        if (eold, enew, enm) != (oold, onew, onm):
            fail(f"event stream of {o}: checksums and NumMembers {(eold, enew, enm)} vs {(oold, onew, onm)}")


def compare_final(eng, ora, c, label):
    n = c["n"]
    where = f"{label} at the end"
    est, einc = eng.rows()
    ost, oinc = ora.rows()
    assert (est == ost).all() and (einc == oinc).all(), f"{where}: {full_diff(eng, ora, n)}"
    for o in range(n):
        assert eng.changes(o) == ora.dis_entries(o), f"{where}: dissemination of {o}"
        assert eng.timers(o) == ora.timer_entries(o), f"{where}: timers of {o}"
        assert eng.iter_state(o) == ora.iter_state(o), f"{where}: iterator of {o}"
        want = {"pingable": ora.num_pingable(o), "maxp": ora.maxp(o), "changes": ora.changes_count(o),
                "members": ora.num_members(o)}
        assert eng.node_stats(o) == want, f"{where}: node_stats of {o}"
    assert (eng.clock_offsets() == ora.clock_offsets()).all(), f"{where}: clock offsets"


def run_case(eng, ora, c, label, after_call=None, after_round=None):
    """the schedule on both sides, compared after every call and at the end; after_call() runs after each compared call,
    after_round(r) after each round of the oracle (fuzz_scenarios.oracle_call)"""
    try:
        _run_case(eng, ora, c, label, after_call, after_round)
    except swimsim.SwimsimError as e:
        if "EHIP" in str(e):                                        # a device error: nothing more runs on this GPU
            pytest.exit(f"{label}: device error, the session ends here: {e}", returncode=3)
        raise


def _run_case(eng, ora, c, label, after_call, after_round=None):
    for o in c["watch"]:
        eng.watch(o, "events")
        ora.watch(o, "events")
    for call in c["calls"]:
        try:
            erets = [x for m, x in ((m, F.apply_mutator(eng, m)) for m in call["muts"]) if m[0] in F.COMPARED_RETURNS]
            eng.step(call["rounds"], call["events"])
        except swimsim.SwimsimError as e:
            if "EHIP" in str(e):
                raise
            pytest.fail(f"{label}: the engine refused: {e}\n{F.describe_call(call)}")
        orets = F.oracle_call(ora, call, after_round=after_round)
        compare_call(eng, ora, c, call, label, erets, orets)
        if after_call:
            after_call()
    assert eng.round == ora.round == c["rounds"]
    compare_final(eng, ora, c, label)


@pytest.mark.parametrize("n,seed", F.CASES, ids=[f"{n}-{s}" for n, s in F.CASES])
def test_random_schedule(n, seed):
    c = F.case(n, seed)
    eng, ora = make_pair(n, init=c["init"], **c["options"])
    try:
        run_case(eng, ora, c, f"case {n}-{seed}")
    finally:
        eng.close()


# ---- tuning variants ("results are identical"): the same schedules, and a counter that shows the variant's path ran ----
# Every (variant, case) pair listed has an observable effect there; the pairs and variants left out have none at these sizes
# (measured on MI355X: the production run of the same case, the variant's run):
#   * hot_slots = 4 is rounded up to one wave of 64 slots. Production fills 65 slots in case 65-1 and 130 in case 130-0,
#     so there the 64 fill up and the other members stay on the dense path; cases 65-0 (64 members ever hot) and 130-1
#     (62) never need a 65th slot.
#   * defer_test = 16 (a one-slot representative table) changes only decisions the table settles: 12 in case 65-0 and 2
#     in case 130-0, none in the seed-1 cases (few deferred decisions, all settled by the direct comparison).
#   * cs_defer = 0 is left out: the default policy skips a round's hashes only when the launch would not fit the
#     side-stream slots (more than 12,288 dirty rows), so at 130 rows the default already hashes every round.
ALL4 = F.VARIANT_CASES
VARIANTS = {"hot_slots0": ({"hot_slots": 0}, ALL4), "hot_slots4": ({"hot_slots": 4}, [(65, 1), (130, 0)]),
            "dense_slots64": ({"dense_slots": 64}, ALL4), "cs_async0": ({"cs_async": 0}, ALL4),
            "cs_narrow_rows0": ({"cs_narrow_rows": 0}, ALL4), "defer_test7": ({"defer_test": 7}, ALL4),
            "defer_test8": ({"defer_test": 8}, ALL4), "defer_test16": ({"defer_test": 16}, [(65, 0), (130, 0)]),
            "cs_defer2": ({"cs_defer": 2}, ALL4)}
VARIANT_RUNS = [(v, n, s) for v, (_, cases) in VARIANTS.items() for (n, s) in cases]


def run_engine_variant(n, seed, tuning, label):
    """case (n, seed) against the oracle under a tuning block; returns kernel_units(), memory() and the largest number
    of hot slots in use after any call (the count drops to 0 at a raw write)"""
    c = F.case(n, seed)
    eng, ora = make_pair(n, init=c["init"], tuning=tuning, **c["options"])
    hot = [0]

    def after_call():
        hot[0] = max(hot[0], int(eng.kernel_units()["hot_slots"]))

    try:
        run_case(eng, ora, c, label, after_call)
        return eng.kernel_units(), eng.memory(), hot[0]
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def production(n, seed):
    """the production engine's counters for case (n, seed): what the variants' counters are compared with"""
    return run_engine_variant(n, seed, None, f"case production-{n}-{seed}")


def took_effect(variant, run, prod):
    """did the tuning variant change how this run's work ran? run, prod = (kernel_units(), memory(), hot slots)"""
    (u, mem, hot), (pu, pmem, phot) = run, prod
    shortcuts = u["defer_rep"] + u["defer_undo"] + u["defer_rep_diff"] + u["defer_undo_diff"]
    return {
        "hot_slots0": lambda: hot == 0 < phot,
        "hot_slots4": lambda: hot == 64 < phot,                    # the pool is full and more members wanted a slot
        "dense_slots64": lambda: mem["dense_cap"] == 64 < pmem["dense_cap"] and mem["lazy_fallbacks"] > 0,
        "cs_async0": lambda: mem["side_cap"] == 0 < pmem["side_cap"],   # no side-stream slots: main-stream launches
        "cs_narrow_rows0": lambda: u["cs_rows_narrow"] == 0 < pu["cs_rows_narrow"] and u["cs_rows_wide"] > 0,
        "defer_test7": lambda: u["defer"] > 0 and shortcuts == 0 and u["defer_norow"] > pu["defer_norow"],
        "defer_test8": lambda: u["lazy_late"] > 0 == pu["lazy_late"],   # senders past the 2-entry log rebuild their rows
        "defer_test16": lambda: u["defer_rep"] + u["defer_rep_diff"] < pu["defer_rep"] + pu["defer_rep_diff"],
        "cs_defer2": lambda: u["cs_skipped_rounds"] > 0 == pu["cs_skipped_rounds"],
    }[variant]()


@pytest.mark.parametrize("variant,n,seed", VARIANT_RUNS, ids=[f"{v}-{n}-{s}" for v, n, s in VARIANT_RUNS])
def test_random_schedule_variants(variant, n, seed):
    run = run_engine_variant(n, seed, VARIANTS[variant][0], f"case {variant}-{n}-{seed}")
    prod = production(n, seed)
    print(f"{variant}-{n}-{seed}: units { {k: v for k, v in run[0].items() if v} } hot slots {run[2]} memory {run[1]}")
    assert took_effect(variant, run, prod), f"{variant} left no trace in this run: {run}\nproduction: {prod}"


@pytest.mark.parametrize("n,seed", F.VARIANT_CASES, ids=[f"{n}-{s}" for n, s in F.VARIANT_CASES])
@pytest.mark.parametrize("shards", [2, 3])
def test_random_schedule_sharded(shards, n, seed):
    """the same schedules over 2 and 3 shards (65 over 3 is uneven); a sharded cluster refuses the direct heal call, so
    those heals run as events"""
    c = F.without_direct_heal(F.case(n, seed))
    eng = swimsim.ShardedCluster(n, shards, init=c["init"], **c["options"])
    try:
        ora = OracleSim(n, init=c["init"], **c["options"])
        run_case(eng, ora, c, f"case {shards}-{n}-{seed}")
    finally:
        eng.close()
