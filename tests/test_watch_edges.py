"""The applied-change streams (swimsim_watch, swimsim_applied_changes, swimsim_applied_events) where the rest of the
suite does not reach: the coalesced drain kernel past one member per thread (N > 1,024), all 64 watch slots with a
refused 65th, a slot given up and taken again, mode switches, the overflow of the per-Update log and caller buffers
shorter than the drain. Engine against OracleSim, bit-exact, compared as tests/test_events.py compares drains; the
scenarios are tests/watch_scenarios.py, and tests/test_watch_edges_host.py shows on the oracle alone that each reaches
its path. A drain changes nothing in the round's state, so no checksum or digest comparison elsewhere notices a wrong one.

A device error (EHIP) ends the session, as in tests/test_fuzz.py: nothing more runs on the GPU after one.
"""
import ctypes as C
import functools
from contextlib import closing

import numpy as np
import pytest

import fuzz_scenarios as F
import swimsim
import watch_scenarios as S
from test_engine_parity import make_pair
from test_events import _drains_match, _events_match
from test_fuzz import run_case

pytestmark = pytest.mark.gpu

EINVAL, EHIP = -1, -3                            # SWIMSIM_EINVAL, SWIMSIM_EHIP


def ends_at_a_device_error(test):
    @functools.wraps(test)
    def run(*a, **kw):
        try:
            return test(*a, **kw)
        except swimsim.SwimsimError as e:
            if "EHIP" in str(e):
                pytest.exit(f"{test.__name__}: device error, the session ends here: {e}", returncode=3)
            raise
    return run


def refused(call, code):
    """the text of the SwimsimError `code` that call() must raise"""
    with pytest.raises(swimsim.SwimsimError) as ei:
        call()
    msg = str(ei.value)
    if "EHIP" in msg:
        raise ei.value
    assert msg.startswith(code), msg
    return msg


def same_round_state(eng, ora, what):
    assert (eng.checksums() == ora.checksums()).all(), f"{what}: checksums"
    assert eng.digest() == ora.digest(), f"{what}: digests"


def changes_of(events):
    return sum(len(ev) for ev in events)


# ---- A: drains past one member per thread ----
@pytest.mark.parametrize("n", S.JOIN_SIZES)
@ends_at_a_device_error
def test_join_list_drains_past_one_member_per_thread(n):
    """dense and exact, no rounds: every thread's run full, a 40 % mix of empty, partial and full runs, then the first
    and the last run alone; the per-Update log takes up to N - 1 changes in one Update"""
    o = S.join_observer(n)
    eng, ora = make_pair(n)
    with closing(eng):
        eng.watch(o, "events")
        ora.watch(o, "events")
        for i, (ms, inc) in enumerate(S.join_lists(n)):
            got, want = S.apply_join_list(eng, o, ms, inc), S.apply_join_list(ora, o, ms, inc)
            assert got == want == len(ms), f"list {i}: {got} applied on the engine, {want} in the oracle"
            _drains_match(eng, ora, (o,))
            _events_match(eng, ora, (o,))
        assert eng.digest() == ora.digest()


@pytest.mark.parametrize("n", S.ROUNDS_SIZES)
@ends_at_a_device_error
def test_round_drains_past_one_member_per_thread(n):
    obs = S.rounds_observers(n)
    eng, ora = make_pair(n)
    with closing(eng):
        for o in obs:
            eng.watch(o, "events")
            ora.watch(o, "events")
        for r0, k, ev in S.calls(S.ROUNDS_STEPS, S.rounds_events(n)):
            eng.step(k, ev)
            for r in range(r0, r0 + k):
                ora.step([e for e in ev if e[0] == r])
            same_round_state(eng, ora, f"after round {r0 + k - 1}")
            _events_match(eng, ora, obs)
            _drains_match(eng, ora, obs)


@pytest.mark.parametrize("n,seed", S.FUZZ_CASES, ids=[f"{n}-{s}" for n, s in S.FUZZ_CASES])
def test_random_schedule_past_one_member_per_thread(n, seed):
    """every event kind, the raw mutators and two watched per-Update streams at N = 1,100 (test_fuzz.run_case; the
    self-only case spends most of its time in the oracle's full syncs)"""
    c = F.case(n, seed)
    eng, ora = make_pair(n, init=c["init"], **c["options"])
    with closing(eng):
        run_case(eng, ora, c, f"case {n}-{seed}")


# ---- B: slots ----
def drain_slots(eng, ora, skip=()):
    obs = [o for o in S.SLOTS_WATCHED if o not in skip]
    _drains_match(eng, ora, obs)
    _events_match(eng, ora, [o for o in obs if S.slots_mode(o) == "events"])


@ends_at_a_device_error
def test_all_64_slots_a_refused_65th_reuse_and_mode_switches():
    wl = S.slots_workload()
    eng, ora = make_pair(wl.n)
    with closing(eng):
        for o in S.SLOTS_WATCHED:
            eng.watch(o, S.slots_mode(o))
            ora.watch(o, S.slots_mode(o))
        # a 65th observer is refused and nothing changes
        digest, memory = eng.digest(), eng.memory()
        for mode in (True, "events"):
            msg = refused(lambda: eng.watch(S.SLOTS_EXTRA, mode), "ECAPACITY")
            assert str(S.WATCH_SLOTS) in msg
        assert eng.digest() == digest == ora.digest() and eng.memory() == memory
        refused(lambda: eng.applied_changes(S.SLOTS_EXTRA), "EINVAL")
        # rounds 0-9, every stream drained each round but those of 5 and 63
        for r in range(10):
            eng.step(1, wl.events_for(r))
            ora.step(wl.events_for(r))
            same_round_state(eng, ora, f"after round {r}")
            drain_slots(eng, ora, skip=S.SLOTS_UNDRAINED)
        # 5 gives its slot up with changes still logged; 100 takes it
        gone, new = S.SLOTS_GIVEN_UP, S.SLOTS_REUSER
        eng.watch(gone, False)
        ora.watch(gone, False)
        eng.watch(new, "events")
        ora.watch(new, "events")
        cs_new = ora.checksum(new)
        assert eng.checksum(new) == cs_new
        assert "not watched" in refused(lambda: eng.applied_changes(gone), "EINVAL")
        refused(lambda: eng.applied_events(gone), "EINVAL")
        with pytest.raises(ValueError):
            ora.drain_applied(gone)
        with pytest.raises(ValueError):
            ora.drain_events(gone)
        # rounds 10-19 in one call; the switcher stays undrained from here on
        eng.step(10, [e for e in wl.events if 10 <= e[0] < 20])
        for r in range(10, 20):
            ora.step(wl.events_for(r))
        same_round_state(eng, ora, "after round 19")
        ev, co = eng.applied_events(new), eng.applied_changes(new)
        oev, oco = ora.drain_events(new), ora.drain_applied(new)
        assert ev[0] == [sorted(x) for x in oev[0]] and ev[1:] == oev[1:]        # nothing of 5's leftovers
        assert co == oco
        assert ev[1] == co[1] == cs_new                                          # OldChecksum: at the watch call
        assert co[0], "observer 100 applied nothing in rounds 10-19"
        # 63 after 20 undrained rounds, then everyone else
        _events_match(eng, ora, (63,))
        _drains_match(eng, ora, (63,))
        sw = S.SLOTS_SWITCHER
        drain_slots(eng, ora, skip=(gone, 63, sw))
        # the switcher: "events" -> coalesced only -> "events"
        eng.watch(sw, True)
        ora.watch(sw, True)
        refused(lambda: eng.applied_events(sw), "EINVAL")
        with pytest.raises(ValueError):
            ora.drain_events(sw)
        eng.step(5, [e for e in wl.events if 20 <= e[0] < 25])
        for r in range(20, 25):
            ora.step(wl.events_for(r))
        same_round_state(eng, ora, "after round 24")
        eng.watch(sw, "events")
        ora.watch(sw, "events")
        cs_sw = ora.checksum(sw)
        got = eng.applied_events(sw)
        assert got == ([], cs_sw, cs_sw, ora.num_members(sw)) == ora.drain_events(sw)   # the stream starts empty
        co = eng.applied_changes(sw)
        assert co == ora.drain_applied(sw) and co[0]                             # rounds 10-24, kept over both switches
        # watching an "events" observer as "events" again keeps its stream (rounds 20-24 are undrained)
        eng.watch(S.SLOTS_REARMED, "events")
        ora.watch(S.SLOTS_REARMED, "events")
        ev, oev = eng.applied_events(S.SLOTS_REARMED), ora.drain_events(S.SLOTS_REARMED)
        assert oev[0] and ev[0] == [sorted(x) for x in oev[0]] and ev[1:] == oev[1:]
        drain_slots(eng, ora, skip=(gone, sw))
        _events_match(eng, ora, (new, sw))
        _drains_match(eng, ora, (new, sw))
        # five more rounds with the new assignment of slots
        for r in range(25, 30):
            eng.step(1, wl.events_for(r))
            ora.step(wl.events_for(r))
            same_round_state(eng, ora, f"after round {r}")
            drain_slots(eng, ora, skip=(gone,))
            _events_match(eng, ora, (new,))
            _drains_match(eng, ora, (new,))


@ends_at_a_device_error
def test_watch_refuses_other_values_of_on_before_it_allocates():
    L = swimsim.load_library()
    eng, ora = make_pair(S.OVERFLOW_N)
    with closing(eng):
        memory, digest = eng.memory(), eng.digest()
        for on in (3, -1, 64, -2 ** 31, 2 ** 31 - 1):
            assert L.swimsim_watch(eng.h, 0, on) == EINVAL, on
            assert b"on is 0, 1 or 2" in L.swimsim_last_error(eng.h)
        assert eng.memory() == memory and eng.digest() == digest                  # no slot, no log
        assert "not watched" in refused(lambda: eng.applied_changes(0), "EINVAL")
        # on a watched observer a refused value leaves the mode and the stream as they are
        eng.watch(0, "events")
        ora.watch(0, "events")
        assert eng.make_change(0, 5, S.T0_MS + S.PERIOD_MS, S.ALIVE) == 1
        assert ora.make_change(0, 5, S.T0_MS + S.PERIOD_MS, S.ALIVE) == 1
        memory = eng.memory()
        assert L.swimsim_watch(eng.h, 0, 3) == EINVAL
        assert eng.memory() == memory
        _events_match(eng, ora, (0,))
        _drains_match(eng, ora, (0,))


# ---- C: overflow of the per-Update log ----
def overflow_pair():
    eng, ora = make_pair(S.OVERFLOW_N)
    for o in S.OVERFLOW_WATCHED:
        eng.watch(o, "events")
        ora.watch(o, "events")
    return eng, ora


def fill_by_join_lists(eng, ora, calls):
    for i in range(1, calls + 1):
        got, want = S.overflow_call(eng, i), S.overflow_call(ora, i)
        assert got == want == len(S.OVERFLOW_MEMBERS), f"call {i}: {got} vs {want}"
    return calls * len(S.OVERFLOW_MEMBERS)


@ends_at_a_device_error
def test_event_log_filled_to_its_last_entry_drains():
    cap = S.event_log_capacity(S.OVERFLOW_N)
    eng, ora = overflow_pair()
    with closing(eng):
        total = fill_by_join_lists(eng, ora, S.OVERFLOW_FILL_CALLS)
        when = S.T0_MS + (S.OVERFLOW_FILL_CALLS + 1) * S.PERIOD_MS
        assert eng.make_change(0, 1, when, S.ALIVE) == ora.make_change(0, 1, when, S.ALIVE) == 1
        assert total + 1 == cap
        ev = eng.applied_events(0)
        oev = ora.drain_events(0)
        assert len(ev[0]) == S.OVERFLOW_FILL_CALLS + 1 and changes_of(ev[0]) == cap
        assert ev[0] == [sorted(x) for x in oev[0]] and ev[1:] == oev[1:]
        _drains_match(eng, ora, S.OVERFLOW_WATCHED)
        _events_match(eng, ora, S.OVERFLOW_WATCHED)
        assert eng.digest() == ora.digest()


def after_the_refusal(eng, ora, rounds, events):
    """every watched per-Update stream whose undrained count in the oracle is past the capacity must be refused and
    restart, the others must match; then the coalesced drains, the digests and `rounds` rounds in parity. Returns the
    refused observers. (OracleSim.drain_events returns up to 4 N + 4096 changes, more than the capacity.)"""
    cap = S.event_log_capacity(S.OVERFLOW_N)
    over = []
    for o in S.OVERFLOW_WATCHED:
        cs = ora.checksum(o)
        x = ora.drain_events(o)                                                   # (discarded where the engine refuses)
        if changes_of(x[0]) <= cap:
            e = eng.applied_events(o)
            assert e[0] == [sorted(ev) for ev in x[0]] and e[1:] == x[1:], f"observer {o}"
            continue
        over.append(o)
        msg = refused(lambda: eng.applied_events(o), "ECAPACITY")
        assert f"observer {o} " in msg and str(cap) in msg, msg
        got = eng.applied_events(o)
        assert got == ([], cs, cs, ora.num_members(o)) == ora.drain_events(o)     # restarted at the refused drain
    _drains_match(eng, ora, S.OVERFLOW_WATCHED)                                   # the coalesced logs lost nothing
    same_round_state(eng, ora, "after the refusal")
    r0 = ora.round
    assert eng.round == r0
    seen = 0
    for r in range(r0, r0 + rounds):
        ev = [e for e in events if e[0] == r]
        eng.step(1, ev)
        ora.step(ev)
        same_round_state(eng, ora, f"after round {r}")
        for o in S.OVERFLOW_WATCHED:
            e, x = eng.applied_events(o), ora.drain_events(o)
            assert e[0] == [sorted(ev) for ev in x[0]] and e[1:] == x[1:], f"observer {o}, round {r}"
            seen += changes_of(x[0])
        _drains_match(eng, ora, S.OVERFLOW_WATCHED)
    assert seen > 0
    return over


@ends_at_a_device_error
def test_event_log_overflow_is_refused_and_the_stream_restarts():
    cap = S.event_log_capacity(S.OVERFLOW_N)
    eng, ora = overflow_pair()
    with closing(eng):
        total = fill_by_join_lists(eng, ora, S.OVERFLOW_FILL_CALLS + 1)
        assert total == 4158 > cap
        # observer 0 holds the members 66 periods ahead, so the rounds' changes reach observer 1's streams
        events = [(r, S.EV_REINCARNATE, m, 0) for r in range(1, 10) for m in (1, 7, 30 + r)]
        assert after_the_refusal(eng, ora, 10, events) == [0]


@ends_at_a_device_error
def test_event_log_overflow_inside_one_step_call():
    """every other member reincarnates in every round of one step call; which logs are past the capacity afterwards is
    read from the oracle's undrained counts (both, 4,257 and 4,339 changes: tests/test_watch_edges_host.py)"""
    eng, ora = overflow_pair()
    with closing(eng):
        more = S.overflow_events(S.OVERFLOW_ROUNDS + 10)
        events = [e for e in more if e[0] < S.OVERFLOW_ROUNDS]
        eng.step(S.OVERFLOW_ROUNDS, events)
        for r in range(S.OVERFLOW_ROUNDS):
            ora.step([e for e in events if e[0] == r])
        same_round_state(eng, ora, "after the long call")
        assert 0 in after_the_refusal(eng, ora, 10, more)


# ---- D: short caller buffers ----
SENTINEL = -123456789
COLUMNS = (np.int32, np.int32, np.int64, np.int32, np.int64)       # member, status, inc, source, source inc


def c_drain(eng, o, stream, cap, arrays=True, counts=True, checksums=True):
    """one drain through the C entry point with `cap` and guarded output arrays: (columns, n, nevents, old, new,
    NumMembers), None for what was not asked for"""
    L = swimsim.load_library()
    dts = COLUMNS + ((np.uint32,) if stream == "events" else ())
    cols = [np.full(cap + S.SHORT_GUARD, SENTINEL, np.int64).astype(dt) for dt in dts]
    n, ne, old, new, nm = C.c_size_t(999), C.c_size_t(999), C.c_uint32(), C.c_uint32(), C.c_int32()
    ptrs = [c.ctypes.data if arrays else None for c in cols]
    pn, pne = (C.byref(n), C.byref(ne)) if counts else (None, None)
    pcs = (C.byref(old), C.byref(new)) if checksums else (None, None)
    pnm = C.byref(nm) if counts and checksums else None
    if stream == "events":
        rc = L.swimsim_applied_events(eng.h, o, *ptrs, cap, pn, pne, *pcs, pnm)
    else:
        rc = L.swimsim_applied_changes(eng.h, o, *ptrs, cap, pn, *pcs, pnm)
    if rc == EHIP:
        raise swimsim.SwimsimError(f"EHIP: {L.swimsim_last_error(eng.h).decode()}")
    assert rc == 0, (rc, L.swimsim_last_error(eng.h))
    return (cols, n.value if counts else None, ne.value if counts and stream == "events" else None,
            old.value if checksums else None, new.value if checksums else None, nm.value if pnm else None)


def check_columns(cols, cap, want):
    """the first min(cap, k) entries are the oracle's, every entry behind them is untouched"""
    m = min(cap, len(want))
    for j, col in enumerate(cols):
        assert [int(x) for x in col[:m]] == [w[j] for w in want[:m]], f"column {j}"
        guard = np.full(len(col) - m, SENTINEL, np.int64).astype(col.dtype)
        assert (col[m:] == guard).all(), f"column {j} was written behind entry {m} (cap {cap}, {len(want)} changes)"


@ends_at_a_device_error
def test_short_buffers_get_the_total_and_no_entry_past_cap():
    wl = S.short_workload()
    o = S.SHORT_OBSERVER
    eng, ora = make_pair(wl.n)
    with closing(eng):
        eng.watch(o, "events")
        ora.watch(o, "events")
        for w, (kind, spec) in enumerate(S.SHORT_WINDOWS):
            rounds = range(w * S.SHORT_WINDOW, (w + 1) * S.SHORT_WINDOW)
            eng.step(len(rounds), [e for e in wl.events if e[0] in rounds])
            for r in rounds:
                ora.step(wl.events_for(r))
            oev, *ometa_ev = ora.drain_events(o)
            oco, *ometa_co = ora.drain_applied(o)
            flat = [c + (i,) for i, ev in enumerate(oev) for c in sorted(ev)]
            assert len(oco) >= 3 and len(flat) >= 3
            for stream, want, nev, meta in (("events", flat, len(oev), ometa_ev), ("changes", oco, None, ometa_co)):
                k = len(want)
                if kind == "cap":
                    cap = S.short_cap(spec, k)
                    cols, n, ne, old, new, nm = c_drain(eng, o, stream, cap)
                    assert (n, ne) == (k, nev), f"window {w} {stream}: *n {n} for {k} changes, *nevents {ne} for {nev}"
                    assert [old, new, nm] == meta
                    check_columns(cols, cap, want)
                elif kind == "counts":                                 # every array NULL, a cap that would admit all
                    _, n, ne, old, new, nm = c_drain(eng, o, stream, k, arrays=False, checksums=False)
                    assert (n, ne) == (k, nev)
                else:                                                  # only the checksums
                    cols, n, ne, old, new, nm = c_drain(eng, o, stream, k, arrays=False, counts=False)
                    assert [old, new] == meta[:2]
            # each drain consumed its stream
            assert eng.applied_events(o)[0] == [] and eng.applied_changes(o)[0] == []
            assert ora.drain_events(o)[0] == [] and ora.drain_applied(o)[0] == []
        same_round_state(eng, ora, "at the end")
