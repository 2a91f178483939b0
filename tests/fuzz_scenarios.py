"""Seeded random schedules for the engine-against-oracle fuzz (tests/test_fuzz_host.py on the CPU oracle alone,
tests/test_fuzz.py engine against oracle). TEST INFRASTRUCTURE ONLY: pure Python, no GPU, no oracle import.

case(n, seed) draws everything a run needs from random.Random of (n, seed) alone:
  * options: short state timeouts (suspect 5, faulty 10, tombstone 5 rounds, so suspect -> faulty -> tombstone ->
    evict fits several times into 60 rounds), ping_request_size, max_rfs_jobs, p_factor, the start ("converged" or
    "self") and the engine seed;
  * 60 rounds cut into step calls of 1, 1, 2, 3 or 7 rounds, each with the events of all its rounds. All eight event
    kinds occur, 0..6 per round; with probability 0.3 an event takes the member of the event before it, which is how
    one member gets several events in one round (reincarnate then kill, kill then revive, a clock step between two
    reincarnates, ...), and nothing keeps an event off a member that is dead, has left or was evicted;
  * raw mutators before about 40 % of the calls (never before the first: the mutators before round 0 are what every
    other parity test has): 1, 2 or 8 of set_member, make_change, clear_changes, set_row, add_join_list, set_live,
    set_partition, set_clock_offset and a direct heal.
Incarnations are t0 + e * period with 0 <= e <= round + 2; partition labels 0, 1, 2; clock offsets -3..3 periods,
and one step of 30 periods per case (backward when the round allows it, so that no clock reads before t0).

Restrictions of the generator, each because one side cannot take the input at all:
  * set_member never writes the observer's own cell (the issue's rule: a node is always in its own list), so a
    one-member cluster draws another mutator instead;
  * a raw write of UNKNOWN (set_member, set_row) carries incarnation t0: the engine's row word of a non-member holds
    e = 0, it has no place for another value (replay() and OracleSim.set_row pass t0);
  * set_row writes the observer's own cell as alive (a node that does not hold itself alive or leave cannot be
    produced by any Update), at a free incarnation;
  * a join-list change without a source carries source incarnation 0, as the reference's source-less changes do
    (heal_partition.go:75-89): the engine's entry of a source-less change has no source incarnation;
  * a clock offset k at round r has r + k >= 0 (the engine refuses a clock before t0), and add_join_list names every
    member once (MembershipAsChanges lists each member once; the engine refuses a repeat).
No event kind and no mutator is left out.

mass_case(n, seed) is the same schedule over 30 rounds from a converged start, with events that take a fraction of the
cluster merged in (MASS_CASES: 1,100, 2,304 and 4,160 members; tests/test_fuzz_at_size_host.py on the oracle,
tests/test_fuzz_at_size.py engine against committed oracle records, tests/fuzz_records.py the records). Every
restriction above holds there too: the mass events are events, which both sides take on any member.
"""
import random

EV_KILL, EV_REVIVE, EV_REINCARNATE, EV_LEAVE, EV_PARTITION, EV_HEAL, EV_REAP, EV_CLOCK = 1, 2, 3, 4, 5, 6, 7, 8
EVENT_NAMES = {EV_KILL: "kill", EV_REVIVE: "revive", EV_REINCARNATE: "reincarnate", EV_LEAVE: "leave",
               EV_PARTITION: "partition", EV_HEAL: "heal", EV_REAP: "reap", EV_CLOCK: "clock"}
ALIVE, SUSPECT, FAULTY, LEAVE, TOMBSTONE, UNKNOWN = 0, 1, 2, 3, 4, 7
T0_MS = 1_500_000_000_000
PERIOD_MS = 200
ROUNDS = 60
MUTATORS = ("set_member", "make_change", "clear_changes", "set_row", "add_join_list", "set_live", "set_partition",
            "set_clock_offset", "heal")

SIZES = (1, 2, 3, 5, 63, 64, 65, 127, 129, 130, 257)
SEEDS = (0, 1, 2)
CASES = [(n, s) for n in SIZES for s in SEEDS]                     # the committed case list
VARIANT_CASES = [(n, s) for n in (65, 130) for s in (0, 1)]       # a subset of CASES: variants and shards

_EVENT_WEIGHTS = ((EV_KILL, 5), (EV_REVIVE, 5), (EV_REINCARNATE, 3), (EV_LEAVE, 2), (EV_PARTITION, 2), (EV_HEAL, 1),
                  (EV_REAP, 2), (EV_CLOCK, 2))
_MUTATOR_WEIGHTS = (("set_member", 4), ("make_change", 4), ("clear_changes", 1), ("set_row", 2), ("add_join_list", 2),
                    ("set_live", 1), ("set_partition", 1), ("set_clock_offset", 1), ("heal", 1))


def _weighted(rng, table):
    return rng.choices([k for k, _ in table], [w for _, w in table])[0]


def _mutator(rng, n, r):
    """one raw mutator before round r: a tuple (name, args...), incarnations and offsets in periods"""
    e = lambda: rng.randint(0, r + 2)
    o = rng.randrange(n)
    name = _weighted(rng, _MUTATOR_WEIGHTS)
    while name == "set_member" and n == 1:
        name = _weighted(rng, _MUTATOR_WEIGHTS)
    if name == "set_member":
        m = rng.choice([x for x in range(n) if x != o]) if n <= 8 else (o + 1 + rng.randrange(n - 1)) % n
        return (name, o, m, rng.choice((ALIVE, SUSPECT, FAULTY, LEAVE, TOMBSTONE, UNKNOWN)), e())
    if name == "make_change":
        return (name, o, rng.randrange(n), e(), rng.choice((ALIVE, SUSPECT, FAULTY, LEAVE, TOMBSTONE)))
    if name == "set_row":
        known = rng.choice((0.2, 0.9))
        st = [rng.choice((ALIVE, ALIVE, ALIVE, SUSPECT, FAULTY, LEAVE, TOMBSTONE)) if rng.random() < known else UNKNOWN
              for _ in range(n)]
        es = [e() for _ in range(n)]
        st[o] = ALIVE
        return (name, o, tuple(st), tuple(es))
    if name == "add_join_list":
        ms = sorted(rng.sample(range(n), rng.choice((1, min(n, 3), min(n, 40)))))
        return (name, o, tuple(ms), tuple(rng.choice((ALIVE, ALIVE, SUSPECT, FAULTY, LEAVE, TOMBSTONE)) for _ in ms),
                tuple(e() for _ in ms), tuple(rng.choice((-1, rng.randrange(n))) for _ in ms), tuple(e() for _ in ms))
    if name == "set_live":
        return (name, o, rng.random() < 0.6)
    if name == "set_partition":
        return (name, o, rng.choice((0, 1, 2)))
    if name == "set_clock_offset":
        return (name, o, max(-r, rng.randint(-3, 3)))
    return (name, o)                                               # clear_changes, heal


def case(n, seed, rounds=ROUNDS):
    """the schedule of case (n, seed): {"n", "seed", "rounds", "init", "options", "watch", "calls"}; calls[i] =
    {"round": first round, "rounds": count, "muts": mutators before the call, "events": [(round, kind, a, b)]}"""
    rng = random.Random(1_000_003 * n + seed)
    opts = dict(suspect_ms=1000, faulty_ms=2000, tombstone_ms=1000, ping_request_size=rng.choice((1, 2, 3, 8)),
                max_rfs_jobs=rng.choice((1, 5)), p_factor=rng.choice((1, 15)), seed=rng.randrange(1, 1 << 32))
    init = rng.choice(("converged", "self"))
    watch = tuple(sorted(rng.sample(range(n), min(2, n))))
    jump_round = rng.randrange(5, rounds)
    prev = rng.randrange(n)
    calls, r = [], 0
    while r < rounds:
        k = min(rng.choice((1, 1, 2, 3, 7)), rounds - r)
        muts = []
        if r and rng.random() < 0.4:
            muts = [_mutator(rng, n, r) for _ in range(rng.choice((1, 2, 8)))]
        events = []
        for rr in range(r, r + k):
            for _ in range(rng.choice((0, 0, 1, 1, 2, 3, 6))):
                kind = _weighted(rng, _EVENT_WEIGHTS)
                a = prev if rng.random() < 0.3 else rng.randrange(n)
                prev = a
                b = 0
                if kind == EV_PARTITION:
                    b = rng.choice((0, 1, 2))
                elif kind == EV_CLOCK:
                    b = max(-rr, rng.randint(-3, 3))
                events.append((rr, kind, a, b))
            if rr == jump_round:
                a = prev if rng.random() < 0.3 else rng.randrange(n)
                prev = a
                events.append((rr, EV_CLOCK, a, -30 if rr >= 30 and rng.random() < 0.5 else 30))
        calls.append({"round": r, "rounds": k, "muts": muts, "events": events})
        r += k
    return {"n": n, "seed": seed, "rounds": rounds, "init": init, "options": opts, "watch": watch, "calls": calls}


# ---- mass schedules: the same vocabulary with a fraction of the cluster taking part, at sizes past 1,024 members ----
# (tests/test_fuzz_at_size_host.py on the oracle, tests/test_fuzz_at_size.py engine against committed oracle records)
MASS_ROUNDS = 30
MASS_CASES = [(1100, 0), (2304, 0), (4160, 0), (4160, 1)]
# Round of each mass event; the leaves fall on random rounds. The kill comes before the reincarnation and the
# reincarnation takes 97 % of the members so that a member revived at round 16 has missed nearly every other member's
# new incarnation: it then changes more than 1,024 cells of its row in one round even at 1,100 members (1,091 on the
# oracle; with 55 % reincarnated after the kill the most was 967).
MASS_KILL_ROUND, MASS_REINCARNATE_ROUND, MASS_CUT_ROUND, MASS_JOIN_ROUND, MASS_HEAL_ROUND = 1, 2, 6, 13, 14
MASS_REVIVE_ROUND, MASS_REAP_ROUND = 16, 18
MASS_REINCARNATE_FRACTION = 0.97


def mass_case(n, seed):
    """case(n, seed, MASS_ROUNDS) from a converged start, with mass events merged into the calls that own their rounds,
    after the base events of the round and in generation order: max(2, n/32) members killed, 97 % of the members
    reincarnated, n/3 members cut off to partition label 1 and joined back, a heal on one member of the cut, every
    second killed member revived, a reap on three observers and four leaves. Deterministic from (n, seed) alone."""
    c = case(n, seed, MASS_ROUNDS)
    c["init"] = "converged"
    rng = random.Random(2_000_003 * n + seed)
    killed = sorted(rng.sample(range(n), max(2, n // 32)))
    reinc = sorted(rng.sample(range(n), int(MASS_REINCARNATE_FRACTION * n)))
    cut = sorted(rng.sample(range(n), n // 3))
    mass = [(MASS_KILL_ROUND, EV_KILL, m, 0) for m in killed]
    mass += [(MASS_REINCARNATE_ROUND, EV_REINCARNATE, m, 0) for m in reinc]
    mass += [(MASS_CUT_ROUND, EV_PARTITION, m, 1) for m in cut]
    mass += [(MASS_JOIN_ROUND, EV_PARTITION, m, 0) for m in cut]
    mass += [(MASS_HEAL_ROUND, EV_HEAL, rng.choice(cut), 0)]
    mass += [(MASS_REVIVE_ROUND, EV_REVIVE, m, 0) for m in killed[::2]]
    mass += [(MASS_REAP_ROUND, EV_REAP, o, 0) for o in rng.sample(range(n), 3)]
    live = [m for m in range(n) if m not in set(killed)]
    mass += [(rng.randrange(MASS_ROUNDS), EV_LEAVE, m, 0) for m in rng.sample(live, 4)]
    calls = []
    for call in c["calls"]:
        events = []
        for r in range(call["round"], call["round"] + call["rounds"]):
            events += [e for e in call["events"] if e[0] == r] + [e for e in mass if e[0] == r]
        calls.append(dict(call, events=events))
    c["calls"] = calls
    return c


def without_direct_heal(c):
    """the same case with every direct heal(o) turned into a heal event, first in the list of the round that follows it
    (a sharded cluster heals through events only)"""
    calls = []
    for call in c["calls"]:
        heals = [(call["round"], EV_HEAL, m[1], 0) for m in call["muts"] if m[0] == "heal"]
        calls.append(dict(call, muts=[m for m in call["muts"] if m[0] != "heal"], events=heals + call["events"]))
    return dict(c, calls=calls)


def inc_of(e):
    return T0_MS + e * PERIOD_MS


def apply_mutator(sim, op):
    """one mutator on an engine (swimsim.Cluster / ShardedCluster) or an OracleSim, which take the same calls; returns
    what the call returns where the two are compared (make_change, add_join_list, heal), else None"""
    name, o = op[0], op[1]
    if name == "set_member":
        _, _, m, st, e = op
        return sim.set_member(o, m, st, inc_of(0 if st == UNKNOWN else e))
    if name == "make_change":
        _, _, m, e, st = op
        return sim.make_change(o, m, inc_of(e), st)
    if name == "clear_changes":
        return sim.clear_changes(o)
    if name == "set_row":
        _, _, st, es = op
        return sim.set_row(o, list(st), [inc_of(0 if s == UNKNOWN else e) for s, e in zip(st, es)])
    if name == "add_join_list":
        _, _, ms, st, es, src, ses = op
        return sim.add_join_list(o, list(ms), list(st), [inc_of(e) for e in es], list(src),
                                 [inc_of(e) if s >= 0 else 0 for s, e in zip(src, ses)])
    if name == "set_live":
        return sim.set_live(o, op[2])
    if name == "set_partition":
        return sim.set_partition(o, op[2])
    if name == "set_clock_offset":
        return sim.set_clock_offset(o, op[2] * PERIOD_MS)
    if name == "heal":
        return sim.heal(o)
    raise ValueError(name)


COMPARED_RETURNS = ("make_change", "add_join_list", "heal")


def oracle_call(ora, call, before_round=None, after_round=None):
    """one step call of the schedule on the oracle: its mutators, then its rounds one by one; returns the compared
    mutator results. before_round(r) and after_round(r) run around each round."""
    rets = [apply_mutator(ora, m) for m in call["muts"]]
    for r in range(call["round"], call["round"] + call["rounds"]):
        if before_round:
            before_round(r)
        ora.step([e for e in call["events"] if e[0] == r])
        if after_round:
            after_round(r)
    return [x for m, x in zip(call["muts"], rets) if m[0] in COMPARED_RETURNS]


def describe_call(call):
    """the events and mutators of one call, for a failure message"""
    ev = ", ".join(f"({r}, {EVENT_NAMES[k]}, {a}, {b})" for (r, k, a, b) in call["events"])
    return (f"call at round {call['round']} ({call['rounds']} rounds): mutators {call['muts']}; events [{ev}]")
