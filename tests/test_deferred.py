"""The deferred full-sync decisions' shortcuts (k_defer_eq), each forced in turn and compared with the CPU
oracle every round.

A receiver whose filtered reply is empty answers with a full sync iff its checksum differs from the sender's issue-time
checksum C_o (disseminator.go:170-180, memberlist.go:367). When one of the two is not known yet the engine defers the
decision and tries to settle it without a hash: (1) a still-clean sender's current row is compared with the receiver's
snapshot, (2) another clean row of checksum C_o is (a checksum representative, k_cs_reps / rep_find), (3) the sender's
row with this phase's logged merges undone is (DS::ulog, wave_rows_differ_undo); (4) otherwise the snapshot is hashed.
A wrong "differ" only costs a hash. A wrong "equal" drops a full sync: the membership then diverges from the
reference's, which shows first in the full_syncs / full_syncs_pingreq counters and then in the checksums.

swimsim_tuning.defer_test (bits 1, 2, 4: skip way 1, 2, 3; 8: undo log of 2 entries; 16: one-slot representative table)
routes the decisions of small workloads through each way. The sizes are no multiples of 64, so the last word of the
divergent-column bitmap is partial and the rows' padding is live. The oracle runs once per workload (oracle_trace) and
every engine run is compared with its record: checksums, state digest and protocol counters after every round.

Two checks on the measurement counters hold in every run (check_units):
  * same decisions in every mode: defer, defer_clean and defer_fs equal those of the all-hashed run (bits 1|2|4), the
    reference behaviour the shortcuts must equal;
  * no false "differ": every decision is settled equal, compared and found different, or not compared (defer_norow). A
    comparison is against the sender's issue-time row, so "different" rows have different checksums (up to a 2^-32
    collision per decision, and none of these workloads has a tombstone, the one status outside the checksum string):
    each such decision must end as a full sync, defer_fs >= defer - equal - defer_norow. A shortcut that restores the
    wrong word (a log replayed in the wrong order, a stale log) and therefore answers "differ" breaks this even where
    the hash then rescues the protocol state.

Counts observed on MI355X, defer_* of kernel_units() as all/eq/rep/undo/rep_diff/undo_diff/norow/fs/undo_over:
  workload    production (0)         1|4 (representatives)   1|2 (undo)              1|2|4 (hashed)
  churn       58/50/7/1/0/0/0/0/0    58/0/57/0/0/0/1/0/0     58/0/0/58/0/0/0/0/0     58/0/0/0/0/0/58/0/0
  cascade     53/51/2/0/0/0/0/0/0    53/6/47/0/0/0/0/0/0     53/6/0/47/0/0/0/0/0     53/6/0/0/0/0/47/0/0
  partition   67/49/5/0/0/0/13/0/0   67/0/52/0/0/0/15/0/0    67/0/0/0/0/0/67/0/0     67/0/0/0/0/0/67/0/0
  selfstart   332/0/0/0/0/0/1/332/0  332/0/0/0/27/0/2/332/0  332/0/0/0/0/0/29/332/0  332/0/0/0/0/0/29/332/0
  bursts      14/14/0/0/0/0/0/0/0    14/0/14/0/0/0/0/0/0     14/0/0/14/0/0/0/0/0     14/0/0/0/0/0/14/0/0
  rawdiff     11/0/0/0/0/0/0/11/0    11/0/0/0/5/0/0/11/0     11/0/0/0/0/5/0/11/0     11/0/0/0/0/0/5/11/0
  twice       2/1/1/0/0/0/0/0/0      2/1/1/0/0/0/0/0/0       2/1/0/1/0/0/0/0/0       2/1/0/0/0/0/1/0/0
  stale       3/2/0/0/0/0/0/1/0      3/1/1/0/0/0/0/1/0       3/1/0/1/0/0/0/1/0       3/1/0/0/0/0/1/1/0
hot_slots = 0 gives the 1|2 column again. 1|2|8 (log of 2): churn 57 undo, 1 over; partition 2 over, selfstart 1 over, the
others as 1|2. 1|4|16 (one slot): churn rep 0 and 5 in two runs, cascade 4 and 0, rawdiff rep_diff 5, the rest norow.
oneslot (68 decisions, 64 eq by pending senders' snapshots, 4 clean senders): 1|4|16 and 1|4 both 3 rep, 1 norow, 1 fs.
Three shards, 1|4 / 1|2: churn250 20 decisions, 15 rep + 5 norow / 5 undo + 15 norow (remote senders); selfstart10 one
decision. Seven rounds per call, cascade, 1|2: 53 decisions, 21 eq (pending senders), 32 undo.
"""
import functools

import numpy as np
import pytest

from oracle_ffi import OracleSim
import swimsim
from swimsim import workloads as W

pytestmark = pytest.mark.gpu

NO_DIRECT, NO_REP, NO_UNDO, UNDO_CAP2, ONE_SLOT = 1, 2, 4, 8, 16
REP_ONLY, UNDO_ONLY, ALL_HASHED = NO_DIRECT | NO_UNDO, NO_DIRECT | NO_REP, NO_DIRECT | NO_REP | NO_UNDO


def bursts(n=300, rounds=45, every=15):
    """config 5's bursts (long messages: undo logs past the cap, dense messages) over config 2's churn. Bursts alone
    defer nothing: a receiver's reply is empty only when every change it holds came from the sender itself (the filter
    of disseminator.go:161-169), which a failure detector's own declarations are and relayed reincarnations are not."""
    wl, churn = W.config5(n=n, rounds=rounds, every=every), W.config2(n=n, rounds=rounds)
    return W.Workload(f"bursts_churn_n{n}", n, rounds, sorted(wl.events + churn.events), "bursts over 1% churn")


def rawdiff(n=333, rounds=30):
    """Rows that differ in a few columns while nothing is being disseminated: raw row writes (swimsim_set_member, an
    Update applied without gossip) make six observers each see one member as suspect at a later incarnation, four times.
    The written rows are dirty receivers with empty replies, their senders are clean, and at most N/4 columns diverge:
    the shortcuts run their comparison, find the rows different, and the decision ends as a full sync."""
    acts = {r: [("set_member", (37 * i + r) % n, (101 * i + 5 * r + 1) % n, swimsim.SUSPECT, swimsim.T0_MS + 200 * (r + 1))
                for i in range(6)] for r in (2, 8, 14, 20)}
    return W.Workload(f"rawdiff_n{n}", n, rounds, [], "raw writes of a few members in a few rows"), acts


def twice(n=70, horizon=12):
    """One deferred decision whose sender's undo log holds a member twice. Planned on the oracle (ping targets do not
    depend on alive changes): a round r in which S is pinged by exactly A < B and pings T, whom nobody else pings.
    Before round r - 1, S learns a change of member c by MakeChange (source S), so in round r it is clean and sends it;
    T, who has not met it, applies it and its reply is empty after the filter: a deferred decision, equal rows. Before
    round r, A and B learn incarnations 1 and 2 of member m: S applies both in sender order in phase D, and its log
    holds {m, word 0}, {m, word 1}. Its issue-time row has word 0, the first logged one."""
    ora, tg = OracleSim(n), []
    for r in range(horizon):
        ora.step(())
        tg.append(ora.last_targets().copy())
    for r in range(1, horizon):
        for S in range(n):
            pingers = [int(x) for x in np.nonzero(tg[r] == S)[0]]
            T = int(tg[r][S])
            met = {int(tg[r - 1][S])} | {int(x) for x in np.nonzero(tg[r - 1] == S)[0]}
            if len(pingers) != 2 or T in pingers or (tg[r] == T).sum() != 1 or T in met:
                continue
            A, B = pingers
            c, m = [x for x in range(n) if x not in (S, T, A, B) and x not in met][:2]
            acts = {r - 1: [("make_change", S, c, swimsim.T0_MS + 200, swimsim.ALIVE)],
                    r: [("make_change", A, m, swimsim.T0_MS + 200, swimsim.ALIVE),
                        ("make_change", B, m, swimsim.T0_MS + 400, swimsim.ALIVE)]}
            wl = W.Workload(f"twice_n{n}", n, r + 1, [], f"round {r}: {A}, {B} -> {S} -> {T}, members {c}, {m}")
            wl.plan = dict(r=r, S=S, A=A, B=B, T=T, c=c, m=m)
            return wl, acts
    raise AssertionError("no round with the wanted ping pattern")


def stale(n=70, horizon=12):
    """One deferred decision whose sender logged a merge in the round before and receives nothing in the round of the
    decision. Round r - 1: S (who learnt member c by MakeChange before it) is pinged by A alone, who carries incarnation 1
    of member m: S logs {m, word 0}. Before round r a raw write gives T the same word of m, without a change to gossip.
    Round r: nobody pings S; S, clean, sends c and m to T alone; T applies c, its reply is empty, its row equals S's
    issue-time row. S's log of this phase is empty. A count left over from round r - 1 would restore word 0 of m and
    answer "differ" (the counts are cleared when a receive phase starts)."""
    ora, tg = OracleSim(n), []
    for r in range(horizon):
        ora.step(())
        tg.append(ora.last_targets().copy())
    for r in range(1, horizon):
        for S in range(n):
            before = [int(x) for x in np.nonzero(tg[r - 1] == S)[0]]
            T = int(tg[r][S])
            met = {int(tg[r - 1][S])} | set(before)
            if len(before) != 1 or (tg[r] == S).any() or (tg[r] == T).sum() != 1 or T in met:
                continue
            A = before[0]
            c, m = [x for x in range(n) if x not in (S, T, A) and x not in met][:2]
            acts = {r - 1: [("make_change", S, c, swimsim.T0_MS + 200, swimsim.ALIVE),
                            ("make_change", A, m, swimsim.T0_MS + 200, swimsim.ALIVE)],
                    r: [("set_member", T, m, swimsim.ALIVE, swimsim.T0_MS + 200)]}
            wl = W.Workload(f"stale_n{n}", n, r + 1, [], f"round {r - 1}: {A} -> {S}; round {r}: {S} -> {T}; members {c}, {m}")
            wl.plan = dict(r=r - 1, S=S, A=A, T=T, c=c, m=m)
            return wl, acts
    raise AssertionError("no round with the wanted ping pattern")


def oneslot(n=70, horizon=12):
    """One deferred decision that the one-slot representative table settles whichever store wins: every clean row holds
    the sender's C_o when the table is built. Before round r - 1, S learns a change of member c by MakeChange; in that
    round it reaches S's target and S's pingers, and the round's end hashes them all to one checksum, C_o. Before round r
    a raw write gives the same word of c to every other row but T's: those rows are dirty through round r, so they
    store nothing. In round r, S pings T, whom nobody else pings and who has not met c: T applies it, its reply is
    empty, its row equals S's issue-time row. The clean rows are S and those S informed, so the slot holds C_o and the
    row found there equals T's snapshot."""
    ora, tg = OracleSim(n), []
    for r in range(horizon):
        ora.step(())
        tg.append(ora.last_targets().copy())
    for r in range(1, horizon):
        for S in range(n):
            T = int(tg[r][S])
            met = {S, int(tg[r - 1][S])} | {int(x) for x in np.nonzero(tg[r - 1] == S)[0]}
            if (tg[r] == T).sum() != 1 or T in met:
                continue
            c = [x for x in range(n) if x != T and x not in met][0]
            acts = {r - 1: [("make_change", S, c, swimsim.T0_MS + 200, swimsim.ALIVE)],
                    r: [("set_member", o, c, swimsim.ALIVE, swimsim.T0_MS + 200) for o in range(n) if o != T and o not in met]}
            wl = W.Workload(f"oneslot_n{n}", n, r + 1, [], f"round {r}: {S} -> {T}, member {c}, informed {sorted(met)}")
            wl.plan = dict(r=r, S=S, T=T, c=c, watch=T)
            return wl, acts
    raise AssertionError("no round with the wanted ping pattern")


WORKLOADS = {
    "churn": lambda: W.config2(n=1000, rounds=40),
    "cascade": lambda: W.config3(n=1000, rounds=45, kill_round=5),
    "partition": lambda: W.config4(n=333, rounds=90),
    "selfstart": lambda: W.selfstart(n=333, seeds=2, rounds=25),
    "bursts": bursts,
    "rawdiff": rawdiff,
    "twice": twice,
    "stale": stale,
    "oneslot": oneslot,
    # (the sharded cases)
    "churn250": lambda: W.config2(n=250, rounds=40),
    "selfstart10": lambda: W.selfstart(n=10, seeds=2, rounds=40),
}
MAIN = ["churn", "cascade", "partition", "selfstart", "bursts", "rawdiff"]
DECLINES = ("partition", "selfstart")   # more than N/4 divergent columns: the undo comparison declines, the decision hashes


@functools.lru_cache(maxsize=None)
def oracle_trace(key):
    """the workload and the oracle's record of it: (checksums, digest, counters) after every round"""
    wl = WORKLOADS[key]()
    wl, acts = wl if isinstance(wl, tuple) else (wl, {})   # acts: {round: [(method, args...)]} called before that round
    ora = OracleSim(wl.n, init=wl.init)
    for o in range(wl.n):
        for m in wl.seed_members:
            if m != o:
                ora.make_change(o, m, swimsim.T0_MS, 0)
    plan = getattr(wl, "plan", None)
    trace = []
    for r in range(wl.rounds):
        for (f, *args) in acts.get(r, ()):
            getattr(ora, f)(*args)
        if plan and r == plan["r"]:
            ora.watch(plan.get("watch", plan["S"]), "events")
        ora.step(wl.events_for(r))
        if plan and r == plan["r"]:                        # the watched node's Updates of the planned round, in order
            plan["updates"] = ora.drain_events(plan.get("watch", plan["S"]))[0]
            ora.watch(plan.get("watch", plan["S"]), False)
        trace.append((ora.checksums().copy(), ora.digest(), ora.counters()))
    return wl, acts, tuple(trace)


def run_vs_oracle(key, defer_test, *, shards=0, chunk=1, **tuning):
    """one engine run of workload `key` under swimsim_tuning.defer_test, compared with the oracle's record after every
    step call (chunk rounds per call; 1: every round); returns kernel_units()"""
    wl, acts, trace = oracle_trace(key)
    assert chunk == 1 or not acts
    if defer_test:
        tuning["defer_test"] = defer_test
    if shards:
        eng = swimsim.ShardedCluster(wl.n, shards, init=wl.init, tuning=tuning or None)
    else:
        eng = swimsim.Cluster(wl.n, init=wl.init, tuning=tuning or None)
    try:
        for o in range(wl.n):
            for m in wl.seed_members:
                if m != o:
                    eng.make_change(o, m, swimsim.T0_MS, swimsim.ALIVE)
        r = 0
        while r < wl.rounds:
            k = min(chunk, wl.rounds - r)
            for (f, *args) in acts.get(r, ()):
                getattr(eng, f)(*args)
            eng.step(k, [e for e in wl.events if r <= e[0] < r + k])
            r += k
            cs, digest, counters = trace[r - 1]
            ec = eng.counters()
            fs = {f: (ec[f], counters[f]) for f in ("full_syncs", "full_syncs_pingreq")}
            assert ec == counters, f"{key} defer_test {defer_test} round {r - 1}: counters differ, full syncs {fs}"
            bad = np.nonzero(eng.checksums() != cs)[0]
            assert len(bad) == 0, f"{key} defer_test {defer_test} round {r - 1}: {len(bad)} checksums differ, rows {bad[:5]}"
            assert eng.digest() == digest, f"{key} defer_test {defer_test} round {r - 1}: state digest differs"
        return eng.kernel_units()
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _units(key, defer_test, hot_slots):
    kw = {} if hot_slots is None else {"hot_slots": hot_slots}
    u = run_vs_oracle(key, defer_test, **kw)
    print(key, defer_test, hot_slots, {k: int(v) for k, v in u.items() if k.startswith("defer")})
    return u


def units(key, defer_test, hot_slots=None):
    """kernel_units() of a single-handle run (one run per case, shared by the tests that read it), checked"""
    u = _units(key, defer_test, hot_slots)
    check_units(key, defer_test, u, _units(key, ALL_HASHED, None) if defer_test != ALL_HASHED else u)
    return u


def check_units(key, defer_test, u, ref):
    tag = f"{key} defer_test {defer_test}: {({k: int(v) for k, v in u.items() if k.startswith('defer')})}"
    for k in ("defer", "defer_clean", "defer_fs"):
        assert u[k] == ref[k], f"{k} differs from the all-hashed run's {int(ref[k])}; {tag}"
    equal = u["defer_eq"] + u["defer_rep"] + u["defer_undo"]
    assert u["defer_fs"] >= u["defer"] - equal - u["defer_norow"], f"a comparison said differ, the checksums equal; {tag}"
    if defer_test & NO_DIRECT:
        # no clean sender's decision is settled by the direct compare: what is left are the pending senders' snapshots
        assert u["defer_eq"] == ref["defer_eq"], f"defer_eq for clean senders; {tag}"
    if defer_test & NO_REP:
        assert u["defer_rep"] == 0 and u["defer_rep_diff"] == 0, tag
    if defer_test & NO_UNDO:
        assert u["defer_undo"] == 0 and u["defer_undo_diff"] == 0 and u["defer_undo_over"] == 0, tag


# ---- the cases -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", MAIN)
def test_all_hashed_reference(key):
    """bits 1|2|4: no shortcut for a clean sender, every such decision hashes the receiver's snapshot"""
    u = units(key, ALL_HASHED)
    assert u["defer"] > 0, u
    assert u["defer_norow"] == u["defer_clean"], u


@pytest.mark.parametrize("key", MAIN)
def test_production_mix(key):
    u = units(key, 0)
    assert u["defer"] > 0, u


@pytest.mark.parametrize("key", MAIN)
def test_representatives_only(key):
    u = units(key, REP_ONLY)
    if key in ("churn", "cascade"):
        assert u["defer_rep"] > 0, u


@pytest.mark.parametrize("hot_slots", [None, 0])
@pytest.mark.parametrize("key", MAIN)
def test_undo_only(key, hot_slots):
    """hot_slots = 0: the logged old words come from the row, not from the hot copy"""
    u = units(key, UNDO_ONLY, hot_slots)
    if key in DECLINES:
        assert u["defer_norow"] > 0, u
    elif key == "rawdiff":                       # (every decision's rows differ)
        assert u["defer_undo_diff"] > 0, u
    else:
        assert u["defer_undo"] > 0, u


@pytest.mark.parametrize("key", MAIN)
def test_undo_cap_2(key):
    """(the scripted decision of twice() stays within the cap of 2: test_member_logged_twice...)"""
    u = units(key, UNDO_ONLY | UNDO_CAP2)
    if key == "churn":
        assert u["defer_undo"] > 0 and u["defer_undo_over"] > 0, u


@pytest.mark.parametrize("key", MAIN)
def test_one_slot_representative_table(key):
    """Every clean row stores into the one slot and the last store wins: which checksum the slot holds is a race by
    design and differs from run to run. A decision's C_o is the checksum of the few rows that already hold the sender's
    news, so it seldom wins: defer_rep was 4 and 0 in two runs of the cascade, 0 and 5 in churn, and cannot be asserted
    without making the test flaky on these workloads (test_one_slot_table_settles_a_decision_as_equal asserts it on a
    scripted decision). What holds in every run: the losers fall through (defer_norow > 0 on churn and cascade), and
    where the clean rows share the senders' checksum (rawdiff) the slot is found and compared."""
    u = units(key, REP_ONLY | ONE_SLOT)
    if key in ("churn", "cascade"):
        assert u["defer_norow"] > 0, u
    if key == "rawdiff":
        assert u["defer_rep"] + u["defer_rep_diff"] > 0, u


@pytest.mark.parametrize("defer_test", [REP_ONLY | ONE_SLOT, REP_ONLY])
def test_one_slot_table_settles_a_decision_as_equal(defer_test):
    """the scripted decision of oneslot(): T applied exactly the change of c from S in the round (checked on the
    oracle's per-Update stream), every row that is clean when the table is built has S's issue-time checksum, and the
    decision is settled as equal through the table, with one slot as with all"""
    wl, _, _ = oracle_trace("oneslot")
    p = wl.plan
    assert [[(ch[0], ch[3]) for ch in upd] for upd in p["updates"]] == [[(p["c"], p["S"])]], (p, p["updates"])
    u = units("oneslot", defer_test)
    assert u["defer_rep"] > 0 and u["defer_rep_diff"] == 0, u


def test_differ_side_of_each_shortcut_is_seen():
    """the forced runs meet decisions whose rows do differ: each shortcut's "differ" answer, and deferred decisions that
    end as full syncs, on at least one workload each"""
    rep = {k: units(k, REP_ONLY) for k in MAIN}
    undo = {k: units(k, UNDO_ONLY) for k in MAIN}
    assert any(u["defer_rep_diff"] > 0 for u in rep.values()), rep
    assert any(u["defer_undo_diff"] > 0 for u in undo.values()), undo
    assert any(u["defer_fs"] > 0 for u in list(rep.values()) + list(undo.values()))


@pytest.mark.parametrize("defer_test", [REP_ONLY, UNDO_ONLY])
@pytest.mark.parametrize("key", ["churn250", "selfstart10"])
def test_sharded_forced_paths(key, defer_test):
    """three shards: senders of other shards (no local row: the sender >= lo && sender < lo + NL bounds) and the remote
    checksum requests under the forced modes"""
    u = run_vs_oracle(key, defer_test, shards=3)
    assert u["defer"] > 0, u
    equal = u["defer_eq"] + u["defer_rep"] + u["defer_undo"]
    assert u["defer_fs"] >= u["defer"] - equal - u["defer_norow"], u


@pytest.mark.parametrize("defer_test,hot_slots", [(UNDO_ONLY, None), (UNDO_ONLY, 0), (UNDO_ONLY | UNDO_CAP2, None)])
def test_member_logged_twice_restores_the_first_word(defer_test, hot_slots):
    """the scripted decision of twice(): the sender applied member m twice in the phase (checked on the oracle's
    per-Update stream), and the undo path still finds its issue-time row equal to the receiver's snapshot. A replay of
    the log in ascending order restores incarnation 1 instead of 0 and answers "differ" (check_units)."""
    wl, _, _ = oracle_trace("twice")
    p = wl.plan
    applied = [ch[0] for upd in p["updates"] for ch in upd]
    assert applied.count(p["m"]) == 2, (p, p["updates"])
    u = units("twice", defer_test, hot_slots)
    assert u["defer_undo"] >= 1 and u["defer_undo_diff"] == 0 and u["defer_undo_over"] == 0, u


@pytest.mark.parametrize("hot_slots", [None, 0])
def test_sender_without_receives_has_an_empty_log(hot_slots):
    """the scripted decision of stale(): the sender applied member m in the round before (checked on the oracle's
    per-Update stream) and is not a receiver in the decision's phase; with the direct compare skipped it reaches the
    undo branch, whose log must be this phase's, empty"""
    wl, _, _ = oracle_trace("stale")
    p = wl.plan
    assert [ch[0] for upd in p["updates"] for ch in upd] == [p["m"]], (p, p["updates"])
    u = units("stale", UNDO_ONLY, hot_slots)
    assert u["defer_undo"] >= 1 and u["defer_undo_diff"] == 0, u


def test_side_generations_meet_the_undo_path():
    """7 rounds per step call: decisions whose checksums are pending in side-stream slots meet the undo path"""
    u = run_vs_oracle("cascade", UNDO_ONLY, chunk=7)
    assert u["defer_undo"] > 0, u
