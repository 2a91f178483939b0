"""Scenarios that carry incarnations past the checksum formatter's table through every caller-facing entry point
(tests/test_incarnation_table_host.py on the CPU oracle alone, tests/test_incarnation_table.py and tests/test_dist_gpu.py
engine against oracle). TEST INFRASTRUCTURE ONLY: pure Python, no GPU, no oracle import.

The engine formats a member's status ‖ decimal(incarnation) ‖ ';' from a per-handle table indexed by the incarnation step
e (incarnation = t0 + e * period), and its checksum kernels clamp an e past the table instead of refusing it. So a
handle must have grown its table before it hashes a row that holds such an e. Every scenario here writes
incarnations at and past the table's bound through one entry point, on observers of the first shard only, and lets the
protocol carry them to the other observers' rows: a handle that has not grown hashes a clamped record there.

TABLES["small"]: max_rounds = 16, so the table has 16 entries until the round counter grows it at round 15. The
incarnation steps are 15 (the last covered entry), 16 (the first uncovered one), 17, 32 and 40. t0 = 10^13 - 40 periods
makes e = 40 the first 14-digit incarnation: its record is a byte longer than any the 16-entry table holds, so a clamped
record has the wrong length as well as the wrong digits.
TABLES["default"]: the default table of 65,536 entries, e = 65,535, 65,536 and 65,539.

One scenario per entry point, the write made before round 0 and again, by other observers on other members, before
round 4; every write is made by observers below 30, rows of the first shard in every split of SPLITS:
  make_change    20 observers declare six members alive, suspect, faulty, leave and tombstone: the changes enter the
                 dissemination buffers and travel as gossip change records;
  set_member     the same cells written raw: nothing to disseminate, the differing checksums start full syncs;
  set_row        8 observers' whole rows at large incarnations: each differs from every other observer's row, and the
                 full syncs carry dense rows;
  add_join_list  join lists of 40 members at large incarnations (AddJoinList clears the changes it applies, so these
                 spread by full sync as well), with and without a source;
  clock          what grows the table without a raw write: a clock offset of +30 periods on one observer of every shard
                 and a Reincarnate of each; an EV_CLOCK of +30 periods in the first round of one six-round step call on a
                 member that ten observers suspect, which it refutes at round + 30; set_round(40) and a Reincarnate at
                 e = 40.

scenario(name, n, table) returns {"name", "n", "bound", "t0_ms", "period_ms", "oracle_kw", "engine_kw", "segments"};
segments[i] = {"muts": [(method, args...)] applied before the segment, "rounds", "events": [(round, kind, a, b)],
"one_call": the engine runs the segment's rounds in one step call}. An engine (swimsim.Cluster / ShardedCluster) and an
OracleSim take the same calls, so apply(sim, op) serves both.
"""
EV_KILL, EV_REVIVE, EV_REINCARNATE, EV_LEAVE, EV_PARTITION, EV_HEAL, EV_REAP, EV_CLOCK = 1, 2, 3, 4, 5, 6, 7, 8
ALIVE, SUSPECT, FAULTY, LEAVE, TOMBSTONE, UNKNOWN = 0, 1, 2, 3, 4, 7
PERIOD_MS = 200
T0_MS = 10**13 - 40 * PERIOD_MS
TABLES = {"small": {"bound": 16, "es": (15, 16, 17, 32, 40), "engine_kw": {"max_rounds": 16}},
          "default": {"bound": 65536, "es": (65535, 65536, 65539), "engine_kw": {}}}
NAMES = ("make_change", "set_member", "set_row", "add_join_list", "clock")
RAW_WRITES = NAMES[:4]                           # the scenarios whose writes only the owning shard sees
DENSE = ("set_member", "set_row", "add_join_list")   # spread by full sync: a dense payload carries the incarnation
SPLITS = {65: (1, 2), 130: (1, 3)}               # uneven splits, the shapes of the fuzz and address-width tests
SHARDED = {65: 2, 130: 3}
OPTIONS = dict(t0_ms=T0_MS, period_ms=PERIOD_MS, suspect_ms=1000, faulty_ms=2000, tombstone_ms=1000, seed=7)
SECOND_WRITE = 4                                 # round before which the second batch of writes is made
ROUNDS = 18                                      # of every raw-write scenario: past round 15, where the small table grows
OWNED = ("make_change", "set_member", "set_row", "add_join_list", "clear_changes")   # calls on the owner of observer op[1]
COMPARED_RETURNS = ("make_change", "add_join_list")
STATUSES = (ALIVE, SUSPECT, FAULTY, LEAVE, ALIVE, TOMBSTONE)


def shard_range(n, shards, rank):
    """observer rows of shard `rank` (the canonical split of include/swimsim.h)"""
    return n * rank // shards, n * (rank + 1) // shards


def _pairs(es, shift):
    """six (incarnation step, status) pairs: every step of the table, the last one twice so that it is hashed (a
    tombstone's record is not); `shift` rotates the statuses, so the second write pairs each step with another status"""
    return [(es[min(i, len(es) - 1)], STATUSES[(i + shift) % len(STATUSES)]) for i in range(len(STATUSES))]


def _cells(n, es, inc, batch):
    """the (observer, member, incarnation, status) cells of write `batch` (0 or 1) of make_change and set_member"""
    writers = range(20) if batch == 0 else range(20, 30)
    first = n - 1 - 6 * batch
    return [(o, first - i, inc(e), st) for o in writers for i, (e, st) in enumerate(_pairs(es, batch))]


def _row(n, o, es, inc):
    st = [SUSPECT if m % 16 == 5 else FAULTY if m % 16 == 11 else UNKNOWN if m % 16 == 14 else ALIVE for m in range(n)]
    ic = [T0_MS if st[m] == UNKNOWN else inc(es[(m + o) % len(es)]) for m in range(n)]
    st[o], ic[o] = ALIVE, inc(es[-1] + 1)
    return st, ic


def _join_list(n, o, es, inc, batch):
    ms = list(range(n - 40, n)) if batch == 0 else list(range(n - 60, n - 20))
    st = [(ALIVE, ALIVE, SUSPECT, ALIVE, FAULTY, ALIVE, LEAVE, TOMBSTONE)[(m + o) % 8] for m in ms]
    ic = [inc(es[(m + o + batch) % len(es)]) for m in ms]
    src = [-1 if m % 2 else (m + 1) % n for m in ms]
    sic = [0 if s < 0 else inc(es[(m + 1) % len(es)]) for m, s in zip(ms, src)]
    return ms, st, ic, src, sic


def _muts(name, n, es, inc, batch):
    if name == "make_change":
        return [("make_change", o, m, i, st) for (o, m, i, st) in _cells(n, es, inc, batch)]
    if name == "set_member":
        return [("set_member", o, m, st, i) for (o, m, i, st) in _cells(n, es, inc, batch)]
    if name == "set_row":
        return [("set_row", o) + _row(n, o, es, inc) for o in (range(8) if batch == 0 else range(8, 12))]
    if name == "add_join_list":
        return [("add_join_list", o) + _join_list(n, o, es, inc, batch) for o in (range(20) if batch == 0 else range(20, 30))]
    raise ValueError(name)


def clock_members(n):
    """the clock scenario's cast: one observer of every shard (of 1, 2 or 3) stepped forward, the suspected member"""
    return (1, n // 2 + 1, n - 2), n // 3


def scenario(name, n, table="small"):
    tb = TABLES[table]
    es = tb["es"]
    inc = lambda e: T0_MS + e * PERIOD_MS
    if name == "clock":
        ahead, p = clock_members(n)
        segments = [
            {"muts": [("set_clock_offset", o, 30 * PERIOD_MS) for o in ahead], "rounds": 3,
             "events": [(0, EV_REINCARNATE, o, 0) for o in ahead]},
            {"muts": [("make_change", q, p, T0_MS, SUSPECT) for q in range(2, 12)], "rounds": 6, "one_call": True,
             "events": [(3, EV_CLOCK, p, 30)]},
            {"muts": [("set_round", 40)], "rounds": 8, "events": [(40, EV_REINCARNATE, 5, 0)]},
        ]
    else:
        segments = [{"muts": _muts(name, n, es, inc, 0), "rounds": SECOND_WRITE, "events": []},
                    {"muts": _muts(name, n, es, inc, 1), "rounds": ROUNDS - SECOND_WRITE, "events": []}]
    return {"name": name, "n": n, "table": table, "bound": tb["bound"], "t0_ms": T0_MS, "period_ms": PERIOD_MS,
            "oracle_kw": dict(OPTIONS), "engine_kw": dict(OPTIONS, **tb["engine_kw"]), "segments": segments}


def apply(sim, op):
    """one call on an engine or an OracleSim; returns what it returns"""
    return getattr(sim, op[0])(*op[1:])


def compared(ops, rets):
    """the return values that engine and oracle are compared on"""
    return [x for op, x in zip(ops, rets) if op[0] in COMPARED_RETURNS]


def run_oracle(ora, sc, after_round=None):
    """the scenario on the oracle alone; after_round(segment index, rounds of the segment run so far) after every round;
    returns the compared return values per segment"""
    rets = []
    for i, seg in enumerate(sc["segments"]):
        rets.append(compared(seg["muts"], [apply(ora, op) for op in seg["muts"]]))
        for k in range(seg["rounds"]):
            r = ora.round
            ora.step([e for e in seg["events"] if e[0] == r])
            if after_round:
                after_round(i, k + 1)
    return rets
