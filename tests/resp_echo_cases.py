"""Shapes for the echoed-response tests (tests/test_resp_echo.py on the engine, tests/test_resp_echo_host.py on the CPU
oracle alone). TEST INFRASTRUCTURE ONLY: pure Python, no GPU; the oracle is passed in.

An echo is a response record that repeats what the sender's message has just told the receiver. The
engine leaves such records out of ping and ping-req responses (swimsim_tuning.resp_echo); results are identical.

  * CASCADES: a converged cluster of n members, k of them killed at round 2, 14 rounds. k sits at the edges of the
    echo bitmap's 32-bit words (31, 32, 33; 64, 65) and of the 64 x 4 records a wave merges and walks per batch (256,
    257, 300). The suspect timeout is 5 rounds, so the faulty wave starts inside the 14 rounds: while it spreads, a
    receiver that holds (faulty, inc) gets (suspect, inc), which is no echo, beside the members on which the two rows
    agree, which are. With the default timeout every record of a 14-round cascade is an echo or news to the receiver,
    and an engine that skipped every hot record without comparing words would pass.
  * WALKS: the three walks of IssueAsReceiver. With every buffered member in a hot slot the receiver walks the slots
    (CASCADES); hot_slots = 0 leaves nothing to skip; hot_slots = 64 with 70 buffered members mixes hot and cold entries
    (the presence-bitmap walk while a row's buffer holds at most a quarter of the padded row, which is every row at
    n = 257 and the rows of the onset at n = 130, whose padded row has 192 cells); the churn shapes buffer more than a
    quarter of the members with cold ones among them (the streaming walk).
  * EXCLUSIONS: seeds of tests/fuzz_scenarios.py that reach the two cases the rule must leave alone: an evicted member
    that is still buffered (its record reads tombstone), and a refute on a stepped-back clock by a node that also
    pinged in the round (the refuted incarnation may lie below the one the node sent).
"""
import fuzz_scenarios as F

ROUNDS = 14
KILL_ROUND = 2
CASCADES = [(65, 3), (130, 31), (130, 32), (130, 33), (257, 64), (257, 65), (1100, 256), (1100, 257), (1100, 300)]
SHARDED = [(130, 33), (257, 65)]
CASCADE_OPTS = {"suspect_ms": 1000}                                # 5 rounds of 200 ms


def killed(n, k):
    """k distinct members, spread over the row (member 0 stays)"""
    return [1 + (i * (n - 1)) // k for i in range(k)]


def cascade_events(n, k):
    return [(KILL_ROUND, F.EV_KILL, m, 0) for m in killed(n, k)]


def churn_events(n, k):
    """k members killed at round 2; every third of them comes back at round 6 and refutes what is said about it"""
    ms = killed(n, k)
    return [(KILL_ROUND, F.EV_KILL, m, 0) for m in ms] + [(6, F.EV_REVIVE, m, 0) for m in ms[::3]]


# name -> (n, events, engine tuning, cluster options)
WALKS = {
    "cold-130": (130, cascade_events(130, 33), {"hot_slots": 0}, {}),
    "cold-257": (257, cascade_events(257, 65), {"hot_slots": 0}, {}),
    "mixed-130": (130, cascade_events(130, 70), {"hot_slots": 64}, {}),
    "mixed-257": (257, cascade_events(257, 70), {"hot_slots": 64}, {}),
    "churn-130": (130, churn_events(130, 70), {"hot_slots": 64}, {}),
    "churn-257": (257, churn_events(257, 90), {"hot_slots": 64}, {}),
    # direct pings at the killed members fail from round 2 on: five helpers per failed ping (Q2, Q3)
    "pingreq-130": (130, cascade_events(130, 33), {}, {"ping_request_size": 5}),
}
# the cascades in which, within the 14 rounds, every live row's buffer holds all k killed members at once (the oracle:
# from round 7 at (65, 3), from rounds 11-12 at the others listed). Not so at (257, 64) and at n = 1,100: the last
# killed members are first suspected around round 8, and their records have not reached every row by round 13. There
# the rows still agree on most killed members, which is all an echo needs (echo_pairs below)
ALL_ROWS_FULL = [(65, 3), (130, 31), (130, 32), (130, 33), (257, 65)]

# (n, seed) of fuzz_scenarios.case, found by a search of its committed sizes 63..257 on the oracle
# (tests/test_resp_echo_host.py asserts what they reach)
EVICTED_BUFFERED = [(65, 1), (127, 0), (130, 1)]
STEPPED_BACK_REFUTE = [(65, 0), (127, 0)]
EXCLUSIONS = sorted(set(EVICTED_BUFFERED + STEPPED_BACK_REFUTE))


def all_rows_hold(ora, members):
    """does every live row's dissemination buffer hold every one of members?"""
    want = set(members)
    return all(want <= set(ora.dis_entries(o)) for o in range(ora.n) if ora.live(o))


def evicted_buffered(ora):
    """(observer, member) pairs of live rows whose buffer holds a member the row has evicted"""
    out = []
    for o in range(ora.n):
        if not ora.live(o):
            continue
        st, _ = ora.row(o)
        out += [(o, m) for m in ora.dis_entries(o) if st[m] == F.UNKNOWN]
    return out


def fuzz_premises(ora, c):
    """runs schedule c on the oracle; returns (rounds with an evicted member still buffered in a live row, rounds with
    a refute on a stepped-back clock by a node that pinged in that round and had no event of its own in it)"""
    evicted, refutes = [], []
    state = {}

    def before(r):
        state["inc"] = [ora.row(o)[1][o] for o in range(ora.n)]
        state["refutes"] = ora.counters()["refutes"]

    def after(r):
        if evicted_buffered(ora):
            evicted.append(r)
        if ora.counters()["refutes"] == state["refutes"]:
            return
        off = ora.clock_offsets()
        tg = ora.last_targets()
        touched = {e[2] for call in c["calls"] for e in call["events"] if e[0] == r}
        for o in range(ora.n):
            st, inc = ora.row(o)
            now = ora.t0_ms + r * ora.period_ms + int(off[o])
            if (off[o] < 0 and o not in touched and ora.live(o) and tg[o] >= 0 and inc[o] != state["inc"][o] and
                    inc[o] == now and st[o] == F.ALIVE):
                refutes.append(r)
                break

    for call in c["calls"]:
        F.oracle_call(ora, call, before, after)
    return evicted, refutes


def echo_pairs(ora, prev_rows, prev_dis):
    """after a round: the (sender, target) pairs of its direct pings in which, before the round, both rows buffered some
    member m (not the sender) with the same known, non-tombstone word, the target's entry not from the sender. The
    target's answer then repeats the sender's record for m unless another message of the round raised it first."""
    st, inc = prev_rows
    tg = ora.last_targets()
    n = 0
    for o in range(ora.n):
        t = int(tg[o])
        if t < 0 or not ora.live(o) or not ora.live(t):
            continue
        for m, (_, src, _) in prev_dis[t].items():
            if (m != o and m in prev_dis[o] and src != o and st[o][m] not in (F.UNKNOWN, F.TOMBSTONE) and
                    st[o][m] == st[t][m] and inc[o][m] == inc[t][m]):
                n += 1
                break
    return n
