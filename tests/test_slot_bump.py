"""Bump by slot on the MI355X engine (swimsim_tuning.slot_bump) against the CPU oracle.

A sender whose message was a walk of its hot slots bumps its piggyback counters from a bitmap of the slots it sent,
written at issue, instead of reading its records back from the pool. Nothing may change: every shape runs with the
path on and off, one round per step call, and after every round the checksums, the three state digests, the ping
targets and the 18 counters are compared with the oracle's; at the end the words, dissemination cells (these carry p)
and timers of sampled rows. The two engine runs are then equal in every read-back. The unit bump_by_slot shows the
path: above 0 with it on wherever the shape has walks of the hot slots, 0 in every round in which each live row holds a
member without a slot, 0 without hot columns and with the path off. (The unit counts the bumps of phase Q3 too, one per
failed helper, so over a whole run it is compared with the answered pings plus the helper errors.) Everything is integer
work: the bar is bit-exact.
tests/test_slot_bump_host.py shows on the oracle what the shapes added in tests/slot_bump_cases.py reach.
"""
import functools

import numpy as np
import pytest

import fuzz_scenarios as F
import resp_echo_cases as R
import slot_bump_cases as S
import swimsim
from oracle_ffi import OracleSim
from test_fuzz import run_case

pytestmark = pytest.mark.gpu

SHAPES = {f"cascade-{n}-{k}": (n, R.cascade_events(n, k), {}, R.CASCADE_OPTS) for n, k in R.CASCADES}
SHAPES.update(S.RECORD_WALKS)
SHAPES.update(S.PF1)
SHAPES.update(S.PINGREQ)
# every buffered member has a hot slot in every round: each bump of a message that is not empty is taken by slot
ALL_HOT = [s for s in SHAPES if s.startswith(("cascade", "pingreq")) or s in ("pf1-130-33", "pf1-257-65")]
NO_HOT = [s for s in SHAPES if s.startswith("cold")]


def sampled(n):
    """first, last, the rows around a 64-row boundary and a few killed and live ones in between"""
    return sorted({0, 1, 2, 63, 64, 65, n // 2, n - 2, n - 1} & set(range(n)))


def read_round(sim):
    return (sim.checksums().tobytes(), tuple(sim.digest()), sim.last_targets().tobytes(),
            tuple(sorted(sim.counters().items())))


def read_end(sim, n, oracle):
    out = []
    for o in sampled(n):
        st, inc = sim.row(o)
        out.append((o, st.tobytes(), np.asarray(inc, np.int64).tobytes(),
                    sim.dis_entries(o) if oracle else sim.changes(o), sim.timer_entries(o) if oracle else sim.timers(o)))
    return out


def device_error(e, label):
    if "EHIP" in str(e):                                            # a device error: nothing more runs on this GPU
        pytest.exit(f"{label}: device error, the session ends here: {e}", returncode=3)


@functools.lru_cache(maxsize=None)
def oracle_trace(shape):
    n, ev, _, opts = SHAPES[shape]
    ora = OracleSim(n, **opts)
    rounds = []
    for r in range(S.ROUNDS):
        ora.step([e for e in ev if e[0] == r])
        rounds.append(read_round(ora))
    return rounds, read_end(ora, n, True)


@functools.lru_cache(maxsize=None)
def engine_trace(shape, bump, shards=1):
    """(per-round read-backs, sampled rows at the end, bump_by_slot after every round) of one engine run"""
    n, ev, tuning, opts = SHAPES[shape]
    tuning = dict(tuning, slot_bump=bump)
    eng = swimsim.Cluster(n, tuning=tuning, **opts) if shards == 1 else swimsim.ShardedCluster(n, shards, tuning=tuning, **opts)
    try:
        rounds, by_slot = [], []
        for r in range(S.ROUNDS):
            eng.step(1, [e for e in ev if e[0] == r])
            rounds.append(read_round(eng))
            by_slot.append(int(eng.kernel_units()["bump_by_slot"]))
        return rounds, read_end(eng, n, False), by_slot
    except swimsim.SwimsimError as e:
        device_error(e, f"{shape} slot_bump {bump} shards {shards}")
        raise
    finally:
        eng.close()


def assert_same(got, want, label, what):
    (grounds, gend), (wrounds, wend) = got, want
    names = ("checksums", "digest", "targets", "counters")
    assert len(grounds) == len(wrounds) and len(gend) == len(wend)
    for r, (g, w) in enumerate(zip(grounds, wrounds)):
        for k, name in enumerate(names):
            if g[k] != w[k]:
                detail = f"{g[k]} vs {w[k]}" if name in ("digest", "counters") else ""
                pytest.fail(f"{label}: round {r}: {name} differ from {what} {detail}")
    for g, w in zip(gend, wend):
        for k, name in enumerate(("observer", "status", "incarnations", "dissemination cells", "timers")):
            assert g[k] == w[k], f"{label}: at the end: {name} of row {g[0]} differ from {what}"


@functools.lru_cache(maxsize=None)
def no_hot_walks(shape):
    return S.rounds_without_hot_walks(OracleSim, shape)


def pings_ok(rounds):
    """successful direct pings after each round (the oracle's counter, which the engine's equals)"""
    return [dict(r[3])["pings_ok"] for r in rounds]


def assert_path(shape, on, off, label):
    """bump_by_slot round by round: with the path on, and 0 with it off"""
    ok = pings_ok(on[0])
    print(f"{label}: bump_by_slot per round, on {np.diff([0] + on[2]).tolist()} off {off[2][-1]}; pings_ok {np.diff([0] + ok).tolist()}")
    assert all(x == 0 for x in off[2])
    if shape in NO_HOT:
        assert all(x == 0 for x in on[2])
        return
    assert on[2][-1] > 0
    ctr = dict(on[0][-1][3])
    # (the unit counts a bump per answered ping and one per failed helper; the first two rounds bump empty buffers)
    assert on[2][-1] < ctr["pings_ok"] + ctr["helper_errors"]
    if shape in S.RECORD_WALKS:
        # rows with cold entries take the record path, round by round: in a round in which every live row holds a member
        # without a slot (the oracle says which), pings are answered and bumped, and none of the bumps goes by slot
        quiet = no_hot_walks(shape)
        per_round, ok_round = np.diff([0] + on[2]), np.diff([0] + ok)
        assert quiet and all(ok_round[r] > 0 for r in quiet)
        assert all(per_round[r] == 0 for r in quiet), (quiet, per_round.tolist())


@pytest.mark.parametrize("bump", [1, 0])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_engine_matches_oracle(shape, bump):
    rounds, end, _ = engine_trace(shape, bump)
    assert_same((rounds, end), oracle_trace(shape), f"{shape} slot_bump {bump}", "the oracle")


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_on_equals_off_and_the_path_fires(shape):
    on, off = engine_trace(shape, 1), engine_trace(shape, 0)
    assert_same(on[:2], off[:2], shape, "the run with slot_bump 0")
    assert_path(shape, on, off, shape)


@pytest.mark.parametrize("shape", ["cascade-130-33", "cascade-257-65"])
def test_every_answered_ping_with_a_buffer_bumps_by_slot(shape):
    """in a cascade with a slot for every killed member, every sender whose buffer is not empty walks its hot slots: in
    the last round, when every live row buffers all killed members (resp_echo_cases.ALL_ROWS_FULL), the bumps by slot
    are at least the answered pings (a failed helper adds one)"""
    on = engine_trace(shape, 1)
    ok, by_slot = pings_ok(on[0]), on[2]
    assert by_slot[-1] - by_slot[-2] >= ok[-1] - ok[-2] > 0


@pytest.mark.parametrize("shape", sorted(S.PINGREQ))
def test_ping_req_error_bumps_go_by_slot(shape):
    """phase Q3 bumps once per failed helper (killed helpers): more bumps by slot than answered direct pings"""
    on = engine_trace(shape, 1)
    ctr = dict(on[0][-1][3])
    assert ctr["helper_errors"] > 0
    assert on[2][-1] > 0


@pytest.mark.parametrize("n,k", R.SHARDED, ids=[f"{n}-{k}" for n, k in R.SHARDED])
def test_sharded(n, k):
    """a shard's bitmaps are indexed by its own rows; senders of one shard ping targets of the other"""
    shape = f"cascade-{n}-{k}"
    on, off = engine_trace(shape, 1, 2), engine_trace(shape, 0, 2)
    assert_same(on[:2], oracle_trace(shape), f"{shape} over 2 shards, slot_bump 1", "the oracle")
    assert_same(off[:2], oracle_trace(shape), f"{shape} over 2 shards, slot_bump 0", "the oracle")
    assert all(x == 0 for x in off[2])
    # A shard gives a slot to a member once one of its own rows buffers it, the single handle once any row does: a
    # member the shard's rows first hear of in phase D is cold there until the next round, so a ping-req message issued
    # in between may be a hot walk on the single handle and not on the shard. Never the other way round.
    one = engine_trace(shape, 1)[2]
    assert on[2][-1] > 0 and all(a <= b for a, b in zip(np.diff([0] + on[2]), np.diff([0] + one)))


# ---- evicted members that are still buffered and refutes on stepped-back clocks, in seeded random schedules ----
def run_fuzz(n, seed, bump):
    c = F.case(n, seed)
    eng = swimsim.Cluster(n, init=c["init"], tuning={"slot_bump": bump}, **c["options"])
    ora = OracleSim(n, init=c["init"], **c["options"])
    try:
        run_case(eng, ora, c, f"case {n}-{seed} slot_bump {bump}")
        return int(eng.kernel_units()["bump_by_slot"])
    finally:
        eng.close()


@pytest.mark.parametrize("n,seed", R.EXCLUSIONS, ids=[f"{n}-{s}" for n, s in R.EXCLUSIONS])
def test_random_schedules(n, seed):
    on, off = run_fuzz(n, seed, 1), run_fuzz(n, seed, 0)
    print(f"case {n}-{seed}: bump_by_slot on {on} off {off}")
    assert on > 0 and off == 0


# ---- a bitmap must not outlive its round ----
def three_rounds(sim, oracle, units=None):
    rounds = []
    for r in range(3):
        rets = S.three_mutators(sim, r)
        sim.step(1, []) if not oracle else sim.step([])
        rounds.append(read_round(sim) + (tuple(rets),))
        if units is not None:
            units.append(int(sim.kernel_units()["bump_by_slot"]))
    return rounds, read_end(sim, S.THREE_N, oracle)


@functools.lru_cache(maxsize=None)
def three_oracle():
    """(the oracle's trace, the rows that walk their hot slots in each round)"""
    ora = OracleSim(S.THREE_N)
    expect = []
    real_step = ora.step

    def step(ev):
        expect.append(len(S.slot_bumps_expected(ora)))              # (after the round's mutators, before its step)
        real_step(ev)

    ora.step = step
    return three_rounds(ora, True), expect


@pytest.mark.parametrize("bump", [1, 0])
def test_three_rounds_hot_walk_then_a_cold_member_then_empty_buffers(bump):
    """round A: the senders walk their hot slots (bitmaps valid). Round B: they hold a cold member too, so their messages
    come from the presence-bitmap walk and their bumps read the records: a bitmap of round A read as valid would leave
    the cold member's p behind. Round C: their buffers are empty and phase D puts a fresh entry into slot 0: a bitmap of
    round A read as valid would bump it. The bumps by slot of every round are exactly the rows the oracle names."""
    eng = swimsim.Cluster(S.THREE_N, tuning=dict(S.THREE_TUNING, slot_bump=bump))
    units = []
    try:
        got = three_rounds(eng, False, units)
    except swimsim.SwimsimError as e:
        device_error(e, f"three rounds, slot_bump {bump}")
        raise
    finally:
        eng.close()
    want, expect = three_oracle()
    for r, (g, w) in enumerate(zip(got[0], want[0])):
        for k, name in enumerate(("checksums", "digest", "targets", "counters", "mutator results")):
            assert g[k] == w[k], f"slot_bump {bump}: round {'ABC'[r]}: {name} differ from the oracle"
    for g, w in zip(got[1], want[1]):
        for k, name in enumerate(("observer", "status", "incarnations", "dissemination cells", "timers")):
            assert g[k] == w[k], f"slot_bump {bump}: at the end: {name} of row {g[0]} differ from the oracle"
    per_round = np.diff([0] + units).tolist()
    print(f"slot_bump {bump}: bumps by slot per round {per_round}, hot walks on the oracle {expect}")
    assert per_round == (expect if bump else [0, 0, 0])


def test_the_switch_is_validated():
    with pytest.raises(swimsim.SwimsimError):
        swimsim.Cluster(8, tuning={"slot_bump": 2})
