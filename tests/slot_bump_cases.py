"""Shapes for the bump-by-slot tests (tests/test_slot_bump.py on the engine, tests/test_slot_bump_host.py on the CPU oracle
alone). TEST INFRASTRUCTURE ONLY: pure Python, no GPU; the oracle is passed in.

A sender whose message was a walk of its hot slots bumps its piggyback counters from a bitmap of the slots it sent
instead of reading its records back (swimsim_tuning.slot_bump); results are identical. The shapes of
tests/resp_echo_cases.py cover the bitmap's 64-bit word edges and the batch edges, the rows with cold entries and the
ping-req bumps; the shapes added here:

  * PF1: cascades with p_factor = 1 and a suspect timeout of 5 rounds. maxP is 1 x digits10(members) = 3, so an entry is
    deleted after three sends: by the sender's bump, and by the sender's own receiver walk between its issue and its
    bump (the bump then finds "no entry" under a set bit and must skip it). With hot_slots = 64 and 70 killed members
    the same on rows with cold entries.
  * pingreq-pf1-130: five helpers per failed ping, killed helpers among them: the bumps of phase Q3, several per message.
  * THREE: three rounds, one step call each, with raw mutators between them, on 64 hot slots. Before round A the rows
    SENDERS suspect the 64 members HOT (a walk of the hot slots: bitmaps valid). Before round B they suspect one member
    more, COLD, which finds no free slot (the presence-bitmap walk: the bitmaps of round A must not be read). Before
    round C their buffers are cleared (nothing is sent: nothing may be bumped), and every other row declares HOT[0]
    faulty, so that the pings of round C put a fresh entry, p = 0, into slot 0 of the cleared rows they reach: a bitmap
    of round A read in round C would bump it.
"""
import fuzz_scenarios as F
import resp_echo_cases as R

ROUNDS = R.ROUNDS
PF1_OPTS = {"p_factor": 1, "suspect_ms": 1000}

# name -> (n, events, engine tuning, cluster options)
PF1 = {
    "pf1-130-33": (130, R.cascade_events(130, 33), {}, PF1_OPTS),
    "pf1-257-65": (257, R.cascade_events(257, 65), {}, PF1_OPTS),
    "pf1-mixed-130": (130, R.cascade_events(130, 70), {"hot_slots": 64}, PF1_OPTS),
    "pf1-mixed-257": (257, R.cascade_events(257, 70), {"hot_slots": 64}, PF1_OPTS),
}
PINGREQ = {
    "pingreq-130": R.WALKS["pingreq-130"],
    "pingreq-pf1-130": (130, R.cascade_events(130, 33), {}, {"ping_request_size": 5, "p_factor": 1}),
}
# rows with cold entries, or no hot columns at all: the record path, round by round
RECORD_WALKS = {k: R.WALKS[k] for k in ("mixed-130", "mixed-257", "churn-130", "churn-257", "cold-130")}



def rounds_without_hot_walks(new_oracle, name):
    """the rounds of a RECORD_WALKS shape in which no message can be a walk of the hot slots: every row that is live in
    the round buffered more members than there are hot slots when the round began, so it holds a member without a slot.
    (With the default p_factor nothing leaves a buffer within the 14 rounds, and the round's events and timers only add
    to it, so this holds at both issues of the round.) new_oracle(n, **options) makes the oracle."""
    n, ev, tuning, opts = RECORD_WALKS[name]
    ora = new_oracle(n, **opts)
    out = []
    for r in range(ROUNDS):
        held = [ora.changes_count(o) for o in range(n)]
        ora.step([e for e in ev if e[0] == r])
        if all(held[o] > tuning["hot_slots"] for o in range(n) if ora.live(o)):
            out.append(r)
    return out


# ---- the three-round case ----
THREE_N = 130
THREE_TUNING = {"hot_slots": 64}
SENDERS = list(range(16))
HOT = list(range(40, 104))
COLD = 110
assert len(HOT) == 64 and COLD not in HOT and not set(SENDERS) & set(HOT + [COLD])


def three_mutators(sim, r):
    """the raw mutators before round r of the three-round case, on the engine or the oracle (the same calls); returns
    their results"""
    inc = F.T0_MS
    out = []
    if r == 0:
        out = [sim.make_change(o, m, inc, F.SUSPECT) for o in SENDERS for m in HOT]
    elif r == 1:
        out = [sim.make_change(o, COLD, inc, F.SUSPECT) for o in SENDERS]
    elif r == 2:
        for o in SENDERS:
            sim.clear_changes(o)
        out = [sim.make_change(o, HOT[0], inc, F.FAULTY) for o in range(THREE_N) if o not in SENDERS]
    return out


def slot_bumps_expected(ora):
    """before a round of the three-round case, on the oracle: the rows whose message will be a walk of the hot slots (a
    buffer that is not empty and holds members of HOT only). Nothing is killed and no timer fires in the three rounds, so
    every one of them pings, is answered and bumps once."""
    rows = []
    for o in range(ora.n):
        buf = set(ora.dis_entries(o))
        if buf and buf <= set(HOT):
            rows.append(o)
    return rows
