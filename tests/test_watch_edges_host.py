"""The watch-edge scenarios (tests/watch_scenarios.py) on the CPU oracle alone: every scenario reaches the path it is
written for, whatever the engine does, so that tests/test_watch_edges.py cannot pass without running that path. The
figures in the assertions' comments were measured with this file (pytest -s prints them)."""
import itertools

import pytest

import fuzz_scenarios as F
import watch_scenarios as S
from oracle_ffi import OracleSim


def changes_of(events):
    return sum(len(ev) for ev in events)


def has_full_run(members, n):
    """does one thread of the coalesced drain find every member of a full-length run changed?"""
    c = S.run_length(n)
    return any(size == c == got for size, got in S.run_fill(members, n))


def test_run_geometry_of_the_sizes():
    assert {n: S.run_length(n) for n in S.JOIN_SIZES} == S.JOIN_RUN_LENGTHS
    assert [S.run_length(n) for n in (64, 130, 1024, 1025)] == [1, 1, 1, 2]
    for n in S.JOIN_SIZES + S.ROUNDS_SIZES:
        rs = S.runs(n)
        assert rs[0][0] == 0 and rs[-1][1] == n and all(a[1] == b[0] for a, b in zip(rs, rs[1:]))
        assert len(rs) <= S.DRAIN_THREADS
    assert S.runs(1025)[-1] == (1024, 1025) and S.runs(3073)[-1] == (3072, 3073)      # the clipped last runs
    assert len(S.runs(1100)) == 550                                                   # threads 550..1023 idle
    assert len(S.runs(2100)) == 700 and S.runs(2100)[-1] == (2097, 2100)
    assert S.event_log_capacity(64) == 4096 and S.event_log_capacity(1100) == 4608
    assert S.event_log_capacity(1024) == 4096 and S.event_log_capacity(1025) == 4352


# ---- A1 ----
@pytest.mark.parametrize("n", S.JOIN_SIZES)
def test_join_lists_apply_whole_and_fill_the_runs(n):
    o, c = S.join_observer(n), S.run_length(n)
    ora = OracleSim(n)
    ora.watch(o, "events")
    lists = S.join_lists(n)
    assert [len(ms) for ms, _ in lists] == [n - 1, int(0.4 * n), 2, 1]
    for ms, inc in lists:
        assert S.apply_join_list(ora, o, ms, inc) == len(ms)          # every listed change applies
        coalesced = ora.drain_applied(o)[0]
        events = ora.drain_events(o)[0]
        assert [x[0] for x in coalesced] == sorted(ms)
        assert len(events) == 1 and sorted(events[0]) == coalesced    # one Update, one event
    fill = S.run_fill(lists[0][0], n)
    assert all(got == size - (b <= o < e) for (size, got), (b, e) in zip(fill, S.runs(n)))   # every run, but for o itself
    fill = S.run_fill(lists[1][0], n)
    kinds = {"none": sum(g == 0 for s, g in fill), "some": sum(0 < g < s for s, g in fill),
             "all": sum(g == s == c for s, g in fill)}
    print(f"join lists n={n}: C={c}, {len(fill)} runs, the 40 % list leaves {kinds}")
    assert all(kinds.values()), kinds
    last = len(S.runs(n)) - 1
    assert S.touched_runs(lists[2][0], n) == [0, last] and S.touched_runs(lists[3][0], n) == [last]


# ---- A2 ----
def rounds_profile(n):
    """the ROUNDS scenario on the oracle: (per-Update changes per observer, largest single drain, a drain filled a run)"""
    ora = OracleSim(n)
    obs = S.rounds_observers(n)
    for o in obs:
        ora.watch(o, "events")
    applied, largest, full = dict.fromkeys(obs, 0), 0, False
    for r0, k, ev in S.calls(S.ROUNDS_STEPS, S.rounds_events(n)):
        for r in range(r0, r0 + k):
            ora.step([e for e in ev if e[0] == r])
        for o in obs:
            applied[o] += changes_of(ora.drain_events(o)[0])
            coalesced = ora.drain_applied(o)[0]
            largest = max(largest, len(coalesced))
            full = full or has_full_run([x[0] for x in coalesced], n)
    assert ora.round == sum(S.ROUNDS_STEPS) == 12
    return applied, largest, full


@pytest.mark.parametrize("n", S.ROUNDS_SIZES)
def test_round_drains_are_large_and_fill_a_run(n):
    applied, largest, full = rounds_profile(n)
    print(f"rounds n={n}: applied {applied}, largest single drain {largest}, a full run: {full}")
    assert set(applied.values()) == {int(S.ROUNDS_BURST * n)}          # 330 each at 1,100, 630 each at 2,100
    assert largest > 100                                               # 111 at 1,100, 299 at 2,100
    assert full


# ---- A3 ----
def fuzz_profile(n, seed):
    """(per-Update changes the watched observers drain over the schedule, the largest single drain)"""
    c = F.case(n, seed)
    ora = OracleSim(n, init=c["init"], **c["options"])
    for o in c["watch"]:
        ora.watch(o, "events")
    total = largest = 0
    for call in c["calls"]:
        F.oracle_call(ora, call)
        for o in c["watch"]:
            k = changes_of(ora.drain_events(o)[0])
            total, largest = total + k, max(largest, k)
    return total, largest


def test_fuzz_cases_are_the_ones_described():
    c = F.case(S.FUZZ_N, 0)
    assert c["init"] == "converged" and c["watch"] == (40, 894)
    first_self = next(s for s in itertools.count() if F.case(S.FUZZ_N, s)["init"] == "self")
    assert first_self == S.FUZZ_SELF_SEED
    assert not set(S.FUZZ_CASES) & set(F.CASES)


def test_fuzz_case_carries_large_drains():
    """case 1100-0. The self-only case 1100-6 takes the oracle 19 s, so it is replayed once only, against the engine;
    measured here once: 4,328 per-Update changes, the largest single drain 887."""
    n, seed = S.FUZZ_CASES[0]
    total, largest = fuzz_profile(n, seed)
    print(f"fuzz case {n}-{seed}: {total} per-Update changes, largest single drain {largest}")
    assert total > 0 and largest > 64                                  # 1,170 and 247


# ---- B ----
def test_slots_scenario_reaches_every_step():
    wl = S.slots_workload()
    ora = OracleSim(wl.n)
    for o in S.SLOTS_WATCHED:
        ora.watch(o, S.slots_mode(o))
    assert S.slots_mode(63) == "events" and S.slots_mode(S.SLOTS_SWITCHER) == "events"
    assert S.slots_mode(S.SLOTS_REARMED) == "events" and S.slots_mode(S.SLOTS_GIVEN_UP) == "events"
    drained = set()
    for r in range(10):
        ora.step(wl.events_for(r))
        for o in S.SLOTS_WATCHED:
            if o not in S.SLOTS_UNDRAINED and ora.drain_applied(o)[0]:
                drained.add(o)
                if S.slots_mode(o) == "events":
                    assert ora.drain_events(o)[0]
    assert len(drained) >= 50                                          # 56
    left = len(ora.drain_applied(S.SLOTS_GIVEN_UP)[0])                 # (the oracle's log is freed with the watch)
    assert left > 0                                                    # 32
    ora.watch(S.SLOTS_GIVEN_UP, False)
    ora.watch(S.SLOTS_REUSER, "events")
    with pytest.raises(ValueError):
        ora.drain_applied(S.SLOTS_GIVEN_UP)
    with pytest.raises(ValueError):
        ora.drain_events(S.SLOTS_GIVEN_UP)
    cs = ora.checksum(S.SLOTS_REUSER)
    for r in range(10, 20):
        ora.step(wl.events_for(r))
    ev, old, _, _ = ora.drain_events(S.SLOTS_REUSER)
    co, old2, _, _ = ora.drain_applied(S.SLOTS_REUSER)
    assert old == old2 == cs
    assert len(co) > 0 and changes_of(ev) >= len(co)                   # 44 members
    ev63 = ora.drain_events(63)[0]
    co63 = ora.drain_applied(63)[0]
    ora.drain_events(S.SLOTS_REARMED)                                  # (drained after round 19 as every other one)
    assert len(co63) > 0 and len(ev63) > 1                             # 68 members in 40 events
    sw = S.SLOTS_SWITCHER
    ora.watch(sw, True)
    with pytest.raises(ValueError):
        ora.drain_events(sw)
    for r in range(20, 25):
        ora.step(wl.events_for(r))
    ora.watch(sw, "events")
    ev, old, new, _ = ora.drain_events(sw)
    assert ev == [] and old == new == ora.checksum(sw)                 # the new stream starts empty
    co7 = ora.drain_applied(sw)[0]
    assert len(co7) > 0                                                # 61: rounds 10-24, kept over both switches
    ora.watch(S.SLOTS_REARMED, "events")                               # re-arming keeps the stream
    kept = ora.drain_events(S.SLOTS_REARMED)[0]
    assert kept
    print(f"slots: {len(drained)} observers drained in rounds 0-9, {left} changes left with observer "
          f"{S.SLOTS_GIVEN_UP}, {len(co)} members at {S.SLOTS_REUSER}, observer 63: {len(co63)} members in "
          f"{len(ev63)} events, observer {sw} after the switches: {len(co7)}, re-armed {S.SLOTS_REARMED}: "
          f"{changes_of(kept)} changes kept")


# ---- C ----
def test_join_lists_fill_the_event_log_to_its_last_entry():
    n, cap = S.OVERFLOW_N, S.event_log_capacity(S.OVERFLOW_N)
    assert cap == 4096
    ora = OracleSim(n)
    for o in S.OVERFLOW_WATCHED:
        ora.watch(o, "events")
    total = sum(S.overflow_call(ora, i) for i in range(1, S.OVERFLOW_FILL_CALLS + 1))
    assert total == 4095 == cap - 1
    assert S.overflow_call(ora, S.OVERFLOW_FILL_CALLS + 1) == 63       # the 66th list: 4,158
    ev = ora.drain_events(0)[0]
    assert len(ev) == 66 and changes_of(ev) == 4158 > cap
    co = ora.drain_applied(0)[0]
    assert [x[0] for x in co] == S.OVERFLOW_MEMBERS                    # 63 members, each with its last change
    assert {x[2] for x in co} == {S.T0_MS + 66 * S.PERIOD_MS}
    assert ora.drain_events(1)[0] == [] and ora.drain_applied(1)[0] == []


def test_one_more_change_fills_it_exactly():
    ora = OracleSim(S.OVERFLOW_N)
    ora.watch(0, "events")
    for i in range(1, S.OVERFLOW_FILL_CALLS + 1):
        S.overflow_call(ora, i)
    assert ora.make_change(0, 1, S.T0_MS + 66 * S.PERIOD_MS, S.ALIVE) == 1
    ev = ora.drain_events(0)[0]
    assert len(ev) == 66 and changes_of(ev) == S.event_log_capacity(S.OVERFLOW_N)


def test_rounds_of_reincarnations_overflow_the_log():
    ora = OracleSim(S.OVERFLOW_N)
    for o in S.OVERFLOW_WATCHED:
        ora.watch(o, "events")
    ev = S.overflow_events()
    for r in range(S.OVERFLOW_ROUNDS):
        ora.step([e for e in ev if e[0] == r])
    counts = [changes_of(ora.drain_events(o)[0]) for o in S.OVERFLOW_WATCHED]
    print(f"overflow by rounds: {counts} undrained changes after {S.OVERFLOW_ROUNDS} rounds")
    # both logs overflow, and both counts are exact: OracleSim.drain_events returns up to 4 N + 4096 = 4,352 changes
    cap = S.event_log_capacity(S.OVERFLOW_N)
    assert all(cap < k <= 4 * S.OVERFLOW_N + 4096 for k in counts)     # 4,257 and 4,339


# ---- D ----
def test_short_buffer_windows_hold_three_changes_and_more():
    wl = S.short_workload()
    ora = OracleSim(wl.n)
    ora.watch(S.SHORT_OBSERVER, "events")
    ks = []
    for w in range(len(S.SHORT_WINDOWS)):
        for r in range(w * S.SHORT_WINDOW, (w + 1) * S.SHORT_WINDOW):
            ora.step(wl.events_for(r))
        ev = ora.drain_events(S.SHORT_OBSERVER)[0]
        co = ora.drain_applied(S.SHORT_OBSERVER)[0]
        ks.append((len(co), changes_of(ev), len(ev)))
    print(f"short buffers: (members, changes, events) per window {ks}")
    assert all(k >= 3 and kc >= 3 for k, kc, _ in ks)              # the fewest: 7 members
    assert any(kc > k for k, kc, _ in ks)                              # a member changed twice inside one window
    assert S.short_cap("k-1", 5) == 4 and S.short_cap("k", 5) == 5 and S.short_cap(1, 5) == 1
