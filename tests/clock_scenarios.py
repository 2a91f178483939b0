"""Scenarios of the per-node clock tests (tests/test_clock_offsets_host.py on the CPU oracle, tests/test_clock_offsets.py
engine against oracle). TEST INFRASTRUCTURE ONLY.

Scenario S: 130 members (three 64-member timer blocks, more than one wave of lanes), short state timeouts, and three
kinds of clock trouble:
  * node 7 is stepped back 30 periods below its own incarnation (it reincarnated at round 41): its refutes lose to
    the rumour they refute until its clock passes the old incarnation (the NTP step-back failure);
  * node 70 is stepped forward 25 periods, node 129 back 40 periods;
  * node 3 is stepped forward 12 periods at round 78 while it holds pending suspect timers (members 100, 101 and 20
    died at round 70), so several timers fire in one round.
A partition of 7 and 70 away from the rest (rounds 55-59) makes the others suspect them, which is what they refute.
"""
import swimsim
from swimsim import workloads as W

P = 200
S_N = 130
S_KW = dict(period_ms=P, suspect_ms=5 * P, faulty_ms=8 * P, tombstone_ms=6 * P)
S_START = 40
S_ROUNDS = 90
S_EVENTS = ([(41, W.EV_REINCARNATE, 7, 0), (41, W.EV_REINCARNATE, 70, 0)] +
            [(55, W.EV_PARTITION, 7, 1), (55, W.EV_PARTITION, 70, 1)] +
            [(60, W.EV_PARTITION, 7, 0), (60, W.EV_PARTITION, 70, 0)] +
            [(70, W.EV_KILL, 100, 0), (70, W.EV_KILL, 101, 0), (70, W.EV_KILL, 20, 0)])
# round -> [(observer, offset in periods)], applied before that round runs
S_CLOCKS = {50: [(7, -30), (70, 25), (129, -40)], 78: [(3, 12)]}
S_END = S_START + S_ROUNDS


def s_events_with_clock_events():
    """S's event list with the clock steps as EV_CLOCK events, each first in its round's list"""
    ev = []
    for r in range(S_START, S_END):
        ev += [(r, swimsim.EV_CLOCK, o, k) for (o, k) in S_CLOCKS.get(r, [])]
        ev += [e for e in S_EVENTS if e[0] == r]
    return ev


def oracle_step(ora, events):
    """one oracle round of an event list that may hold EV_CLOCK events: they are stripped and set through
    set_clock_offset before the round (each comes first in its round's list), which checks the engine's event against
    the setter; the oracle's own OR_EV_CLOCK is what tests/test_fuzz.py runs"""
    r = ora.round
    for (er, k, a, b) in events:
        if er == r and k == swimsim.EV_CLOCK:
            ora.set_clock_offset(a, b * ora.period_ms)
    ora.step([e for e in events if e[0] == r and e[1] != swimsim.EV_CLOCK])


def run_oracle_s(skew=True, watch_events=None):
    """scenario S on the oracle alone, with or without its clock steps; returns the oracle"""
    from oracle_ffi import OracleSim
    ora = OracleSim(S_N, **S_KW)
    ora.set_round(S_START)
    if watch_events is not None:
        ora.watch(watch_events, "events")
    for r in range(S_START, S_END):
        if skew:
            for (o, k) in S_CLOCKS.get(r, []):
                ora.set_clock_offset(o, k * P)
        ora.step([e for e in S_EVENTS if e[0] == r])
    return ora
