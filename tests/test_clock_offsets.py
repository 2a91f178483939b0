"""Per-node clock offsets on the MI355X engine against the CPU oracle (docs/ROUND_SEMANTICS.md §2 Clock):
now(o) = t0 + (round + k_o) * period. The oracle has had or_set_clock_offset from the start; every result here is
compared bit for bit, every round unless said otherwise: ping targets, checksums, the three state digests, counters
(test_engine_parity.run_parity, with a full-state diff on a mismatch).

The scenarios are the reference's partition heal with one mock clock per partition (heal_partition_test.go:36-77,
447-454) and scenario S of clock_scenarios.py (a clock stepped back below the node's own incarnation, forward steps
that make several timers due at once)."""
import numpy as np
import pytest

import swimsim
from swimsim import workloads as W
from oracle_ffi import OracleSim
from test_engine_parity import full_diff, make_pair, run_parity
import clock_scenarios as CS

pytestmark = pytest.mark.gpu

P = CS.P


def state_of(c):
    return {"digest": c.digest(), "checksums": [int(x) for x in c.checksums()], "counters": c.counters()}


@pytest.fixture(scope="module")
def s_oracle():
    """scenario S on the oracle, once: its final state, and the refute count of the run without clock steps"""
    return {"final": state_of(CS.run_oracle_s(True)), "plain_refutes": CS.run_oracle_s(False).counters()["refutes"]}


def set_both(eng, ora, o, k):
    eng.set_clock_offset(o, k * P)
    ora.set_clock_offset(o, k * P)


def make_s(shards=0, **kw):
    """engine and oracle at the start of scenario S"""
    if shards:
        eng = swimsim.ShardedCluster(CS.S_N, shards, **CS.S_KW, **kw)
        ora = OracleSim(CS.S_N, **CS.S_KW)
    else:
        eng, ora = make_pair(CS.S_N, **CS.S_KW, **kw)
    try:
        eng.set_round(CS.S_START)
        ora.set_round(CS.S_START)
    except Exception:
        eng.close()
        raise
    return eng, ora


def run_s(eng, ora, check_every=1, until=CS.S_END, after_round=None):
    """S with its clock steps set through set_clock_offset between steps; after_round(r) runs after round r"""
    at = CS.S_START
    while at < until:
        for (o, k) in CS.S_CLOCKS.get(at, []):
            set_both(eng, ora, o, k)
        nxt = min([r for r in CS.S_CLOCKS if r > at] + [until])
        n = 1 if after_round else nxt - at
        run_parity(eng, ora, CS.S_N, n, CS.S_EVENTS, check_every=check_every)
        at += n
        if after_round:
            after_round(at - 1)


def heal_layout(eng, ora, n):
    """each half alive to itself and faulty to the other, buffers cleared (heal_partition_test.go:36-77, as
    test_engine_parity.test_partition_heal_reference_scenario sets it up)"""
    A, B = range(n // 2), range(n // 2, n)
    for part in (A, B):
        for o in part:
            for m in part:
                eng.set_member(o, m, swimsim.ALIVE, swimsim.T0_MS)
                ora.set_member(o, m, 0, swimsim.T0_MS)
    for X, Y in ((A, B), (B, A)):
        for o in X:
            for m in Y:
                eng.make_change(o, m, swimsim.T0_MS, swimsim.FAULTY)
                ora.make_change(o, m, swimsim.T0_MS, 2)
            eng.clear_changes(o)
            ora.clear_changes(o)
    return A, B


def run_heal(n, ka, kb, start_round):
    eng, ora = make_pair(n, init="self")
    try:
        if start_round:
            eng.set_round(start_round)
            ora.set_round(start_round)
        A, B = heal_layout(eng, ora, n)
        offs = np.array([ka * P if o in A else kb * P for o in range(n)], np.int64)
        eng.set_clock_offsets(offs)                                  # the bulk call
        for o in range(n):
            ora.set_clock_offset(o, int(offs[o]))
        ev = [(eng.round, W.EV_HEAL, 0, 0), (eng.round + 30, W.EV_HEAL, 0, 0)]
        run_parity(eng, ora, n, 90, ev)
        assert ora.converged() and eng.converged()
        st, _ = eng.rows()
        assert (st == swimsim.ALIVE).all()
        assert (eng.clock_offsets() == offs).all()
        assert ora.counters()["heal_attempts"] > 0
    finally:
        eng.close()


def test_reference_heal_scenario_with_its_clocks():
    """heal_partition_test.go:36-77 with partition A's clock 3 periods and B's 5 periods ahead (447-454): the
    suspects the heal spreads are refuted with now(o) of each side's own clock, and everyone ends alive everywhere"""
    run_heal(10, 3, 5, 0)


def test_heal_scenario_130_members_back_and_forward_offsets():
    """the same layout at 65 + 65 (rows span three 64-member timer blocks and more than one wave of lanes), A two
    periods behind and B seven ahead, from round 10"""
    run_heal(130, -2, 7, 10)


def test_scenario_s_setters_between_steps(s_oracle):
    eng, ora = make_s()
    try:
        run_s(eng, ora)
        c = eng.counters()
        print(f"refutes {c['refutes']} (no clock steps: {s_oracle['plain_refutes']}), applied {c['applied']}")
        assert c["refutes"] > s_oracle["plain_refutes"]
        assert state_of(eng) == s_oracle["final"]
        want = np.zeros(CS.S_N, np.int64)
        for steps in CS.S_CLOCKS.values():
            for (o, k) in steps:
                want[o] = k * P
        assert (eng.clock_offsets() == want).all()
    finally:
        eng.close()


def test_scenario_s_clock_events_in_multi_round_steps(s_oracle):
    """the clock steps as EV_CLOCK events inside step(10, ...): the oracle strips them and sets its offsets before
    the round; every block ends equal, the end equals the run with setters"""
    eng, ora = make_s()
    try:
        ev = CS.s_events_with_clock_events()
        for r0 in range(CS.S_START, CS.S_END, 10):
            eng.step(10, [e for e in ev if r0 <= e[0] < r0 + 10])
            for _ in range(10):
                CS.oracle_step(ora, ev)
            assert (eng.checksums() == ora.checksums()).all() and eng.digest() == ora.digest(), \
                f"block from round {r0}: {full_diff(eng, ora, CS.S_N)}"
            assert eng.counters() == ora.counters()
        assert eng.round == CS.S_END
        assert state_of(eng) == s_oracle["final"]
    finally:
        eng.close()


@pytest.mark.parametrize("variant", ["hot_slots0", "defer_1_2", "defer_1_4", "cs_async0", "shards2", "shards3"])
def test_scenario_s_under_engine_variants(variant, s_oracle):
    kw = {"hot_slots0": dict(tuning={"hot_slots": 0}), "defer_1_2": dict(tuning={"defer_test": 1 | 2}),
          "defer_1_4": dict(tuning={"defer_test": 1 | 4}), "cs_async0": dict(tuning={"cs_async": 0}),
          "shards2": dict(shards=2), "shards3": dict(shards=3)}[variant]
    eng, ora = make_s(**kw)
    try:
        run_s(eng, ora, check_every=5)
        assert state_of(eng) == s_oracle["final"]
    finally:
        eng.close()


def test_event_stream_order_after_a_forward_step():
    """node 3's forward step at round 78 makes timers with different deadlines due at once: the per-Update stream
    lists them as the oracle fires them, in (deadline, member) order, and every other round's stream matches too"""
    eng, ora = make_s()
    seen = {}
    try:
        eng.watch(3, "events")
        ora.watch(3, "events")

        def compare(r):
            ee, eold, enew, enm = eng.applied_events(3)
            oe, oold, onew, onm = ora.drain_events(3)
            oe = [sorted(x) for x in oe]                             # (one Update's changes: member order)
            assert len(ee) == len(oe), f"round {r}: {len(ee)} events on the engine, {len(oe)} in the oracle"
            for i, (a, b) in enumerate(zip(ee, oe)):
                assert a == b, f"round {r}, event {i}: engine {a} vs oracle {b}"
            assert (eold, enew, enm) == (oold, onew, onm)
            seen[r] = oe

        run_s(eng, ora, until=82, after_round=compare)
        fired = [e for e in seen[78] if len(e) == 1 and e[0][1] in (swimsim.FAULTY, swimsim.TOMBSTONE) and e[0][3] == 3]
        assert len(fired) >= 2, seen[78]
    finally:
        eng.close()


def test_readbacks_are_in_the_owners_clock():
    eng, ora = make_s()
    try:
        run_s(eng, ora, check_every=10)
        for o in (3, 7, 70):
            assert eng.timers(o) == ora.timer_entries(o), f"timers of {o}"
            est, einc = eng.row(o)
            ost, oinc = ora.row(o)
            assert (est == ost).all() and (einc == oinc).all(), f"row of {o}"
    finally:
        eng.close()


def test_errors_change_nothing():
    n = 16
    eng, ora = make_pair(n)
    L = swimsim.load_library()
    try:
        def still_in_step():
            run_parity(eng, ora, n, 2, [(eng.round, W.EV_REINCARNATE, 2, 0)])

        assert L.swimsim_set_clock_offset(eng.h, 0, P // 2) == -5          # not a whole number of periods
        still_in_step()
        assert L.swimsim_set_clock_offset(eng.h, 0, 32768 * P) == -5       # more than 32,767 periods
        assert L.swimsim_set_clock_offset(eng.h, 0, -32768 * P) == -5
        still_in_step()
        assert L.swimsim_set_clock_offset(eng.h, n, 0) == -1               # observer N
        bad = np.zeros(n, np.int64)
        bad[n - 1] = P // 2
        assert L.swimsim_set_clock_offsets(eng.h, bad.ctypes.data) == -5   # the bulk call checks every entry first
        assert L.swimsim_set_clock_offsets(eng.h, None) == -1
        assert L.swimsim_clock_offsets(eng.h, None) == -1
        assert (eng.clock_offsets() == 0).all()
        still_in_step()
    finally:
        eng.close()
    eng, ora = make_pair(n)
    try:
        assert L.swimsim_set_clock_offset(eng.h, 1, -P) == -5              # round 0: a clock before t0
        assert (eng.clock_offsets() == 0).all()
        run_parity(eng, ora, n, 2)
        eng.set_round(20)
        ora.set_round(20)
        set_both(eng, ora, 1, -10)
        assert L.swimsim_set_round(eng.h, 5) == -5                         # 5 - 10 < 0 with that offset in force
        assert eng.round == 20
        with pytest.raises(swimsim.SwimsimError, match="ERANGE"):
            eng.step(3, [(eng.round + 1, swimsim.EV_CLOCK, 0, 40000)])     # checked before any round runs
        assert eng.round == 20
        with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
            eng.step(1, [(eng.round, swimsim.EV_CLOCK, n, 1)])
        assert eng.round == 20 and eng.clock_offsets()[1] == -10 * P
        run_parity(eng, ora, n, 4, [(eng.round + 1, W.EV_REINCARNATE, 1, 0)])
        assert eng.member(1, 1)[1] == swimsim.T0_MS + (21 - 10) * P         # Reincarnate took node 1's own clock
    finally:
        eng.close()


def test_zero_offsets_are_a_no_op():
    wl = W.config2(n=64, rounds=20)
    a, b = swimsim.Cluster(wl.n), swimsim.Cluster(wl.n)
    try:
        a.set_clock_offsets(np.zeros(wl.n, np.int64))
        for r in range(wl.rounds):
            ev = wl.events_for(r)
            a.step(1, ev)
            b.step(1, ev)
            assert a.digest() == b.digest(), f"round {r}"
            assert (a.checksums() == b.checksums()).all(), f"round {r}"
        assert a.counters() == b.counters()
    finally:
        a.close()
        b.close()
