"""Pending-live senders: a sender that is dirty when it issues is not copied. Its issue-time row is its
live row with the receive phase's undo log applied backwards, compared in place by k_defer_eq and rebuilt as a dense
snapshot only when the content would be lost (a receive wave whose log would overflow or that merges a dense message:
lazy_late) or when a decision needs the sender's checksum after all (k_lazy_mat: lazy_mat). Every run is compared with
the CPU oracle after every step call: checksums, state digest, protocol counters. The sizes are no multiples of 64.

The scripted decisions are planned on the oracle (ping targets do not depend on alive changes). Round r: S pings T,
whom nobody else pings. Before round r, S learns a new incarnation of member c by MakeChange, so S is dirty at issue and
sends c; T applies it, and its reply is empty after the filter (its only change came from S): a deferred decision whose
sender is pending, live. T's row then equals S's issue-time row.
  quiet   nobody pings S in round r: its undo log is empty.
  logged  S is pinged by exactly A < B. Before round r, A learns incarnation 1 of member m and of member m2, B
          incarnation 2 of m: S's log is {m, word 0}, {m2, word 0}, {m, word 1}, and its issue-time row holds word 0 of
          m, the first logged one. With a log of 2 entries (defer_test 8) the third change overflows it: S's receive wave
          rebuilds the row from the live row and the three logged words.
  differ  quiet, and a raw write before round r gives T another word of member x: the rows differ, S's checksum is
          needed, k_lazy_mat rebuilds its row, and the decision ends as the oracle's does (a full sync).
"""
import functools

import numpy as np
import pytest

from oracle_ffi import OracleSim
import swimsim
from swimsim import workloads as W
from test_deferred import bursts

pytestmark = pytest.mark.gpu

UNDO_CAP2 = 8


def scripted(kind, n=300, horizon=12):
    ora, tg = OracleSim(n), []
    for r in range(horizon):
        ora.step(())
        tg.append(ora.last_targets().copy())
    want = 2 if kind == "logged" else 0
    for r in range(1, horizon):
        for S in range(n):
            pingers = [int(x) for x in np.nonzero(tg[r] == S)[0]]
            T = int(tg[r][S])
            if len(pingers) != want or T < 0 or T in pingers or (tg[r] == T).sum() != 1:
                continue
            free = [x for x in range(n) if x not in (S, T, *pingers)]
            c, m, m2, x = free[:4]
            acts = [("make_change", S, c, swimsim.T0_MS + 200, swimsim.ALIVE)]
            if kind == "logged":
                A, B = pingers
                acts += [("make_change", A, m, swimsim.T0_MS + 200, swimsim.ALIVE),
                         ("make_change", A, m2, swimsim.T0_MS + 200, swimsim.ALIVE),
                         ("make_change", B, m, swimsim.T0_MS + 400, swimsim.ALIVE)]
            if kind == "differ":
                acts += [("set_member", T, x, swimsim.SUSPECT, swimsim.T0_MS + 200)]
            wl = W.Workload(f"{kind}_n{n}", n, r + 2, [], f"round {r}: {pingers} -> {S} -> {T}")
            wl.plan = dict(r=r, S=S, T=T, pingers=pingers, c=c, m=m)
            return wl, {r: acts}
    raise AssertionError("no round with the wanted ping pattern")


WORKLOADS = {
    "quiet": lambda: scripted("quiet"),
    "logged": lambda: scripted("logged"),
    "differ": lambda: scripted("differ"),
    "cascade": lambda: W.config3(n=1000, rounds=45, kill_round=5),
    "bursts": bursts,
    "selfstart": lambda: W.selfstart(n=300, seeds=2, rounds=25),
    "faulty300": lambda: W.config3(n=300, rounds=63, kill_round=10),
    "faulty333": lambda: W.config3(n=333, rounds=45, kill_round=3),
}


@functools.lru_cache(maxsize=None)
def oracle_trace(key):
    """the workload and the oracle's record of it: (checksums, digest, counters) after every round"""
    wl = WORKLOADS[key]()
    wl, acts = wl if isinstance(wl, tuple) else (wl, {})
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
            ora.watch(plan["S"], "events")
        ora.step(wl.events_for(r))
        if plan and r == plan["r"]:                        # S's Updates of the planned round, in order
            plan["updates"] = ora.drain_events(plan["S"])[0]
            ora.watch(plan["S"], False)
        trace.append((ora.checksums().copy(), ora.digest(), ora.counters()))
    return wl, acts, tuple(trace)


def run_vs_oracle(key, defer_test=0, *, shards=0, chunk=1, **tuning):
    """one engine run compared with the oracle's record after every step call; returns kernel_units()"""
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
        u = eng.kernel_units()
        print(key, defer_test, shards, chunk, {k: int(v) for k, v in u.items() if k.startswith(("defer", "lazy", "issue_"))})
        return u
    finally:
        eng.close()


def test_quiet_pending_sender_is_compared_in_place():
    """S receives nothing in the round: the live row is the issue-time row"""
    wl, _, trace = oracle_trace("quiet")
    assert wl.plan["updates"] == [], wl.plan
    u = run_vs_oracle("quiet")
    assert u["issue_snaps"] == 0 and u["defer"] > 0 and u["defer_eq"] >= 1, u
    assert u["lazy_late"] == 0 and u["lazy_mat"] == 0, u
    assert u["defer_undo"] == 0 and u["defer_undo_diff"] == 0 and u["defer_undo_over"] == 0 and u["defer_norow"] == 0, u


def check_logged_plan():
    wl, _, _ = oracle_trace("logged")
    p = wl.plan
    applied = [ch[0] for upd in p["updates"] for ch in upd]
    assert applied.count(p["m"]) == 2 and len(applied) == 3, (p, p["updates"])


def test_member_logged_twice_restores_the_first_word():
    """S applies member m twice in the round (checked on the oracle's per-Update stream); its issue-time row has the
    first logged word. A replay in ascending order would find the rows different, hash, and count lazy_mat."""
    check_logged_plan()
    u = run_vs_oracle("logged")
    assert u["issue_snaps"] == 0 and u["defer"] > 0 and u["defer_eq"] >= 1, u
    assert u["lazy_late"] == 0 and u["lazy_mat"] == 0, u
    assert u["defer_undo"] == 0 and u["defer_undo_diff"] == 0 and u["defer_undo_over"] == 0 and u["defer_norow"] == 0, u


def test_log_overflow_rebuilds_the_row_in_the_receive_wave():
    """log of 2 entries: the third change S applies overflows it, and the rebuilt row still equals T's snapshot"""
    check_logged_plan()
    u = run_vs_oracle("logged", UNDO_CAP2)
    assert u["issue_snaps"] == 0 and u["lazy_late"] >= 1 and u["lazy_mat"] == 0 and u["defer_eq"] >= 1, u


@pytest.mark.parametrize("key", ["cascade", "bursts"])
def test_forced_late_rebuilds_on_workloads(key):
    u = run_vs_oracle(key, UNDO_CAP2)
    assert u["issue_snaps"] == 0 and u["lazy_late"] > 0, u


def test_dense_messages_into_pending_senders():
    """the self-only start: every sender is dirty at issue and nearly every deferred decision ends as a full sync, so
    the pending senders' rows are rebuilt and hashed (observed on MI355X: 278 decisions, lazy_mat 270, lazy_late 0: the
    full-sync responses are merged in k_resp, after the receive phase, so no receive wave meets a dense message)"""
    u = run_vs_oracle("selfstart", UNDO_CAP2)
    assert u["issue_snaps"] == 0 and u["lazy_late"] + u["lazy_mat"] > 0, u
    u = run_vs_oracle("selfstart")
    assert u["issue_snaps"] == 0 and u["lazy_late"] + u["lazy_mat"] > 0, u


def test_differing_rows_hash_the_rebuilt_sender():
    wl, _, trace = oracle_trace("differ")
    r = wl.plan["r"]
    assert trace[r][2]["full_syncs"] > (trace[r - 1][2]["full_syncs"] if r else 0), wl.plan
    u = run_vs_oracle("differ")                                    # (full_syncs equal the oracle's: every round's parity)
    assert u["issue_snaps"] == 0 and u["lazy_mat"] >= 1 and u["lazy_late"] == 0 and u["defer_fs"] >= 1, u


@pytest.mark.parametrize("shards", [0, 3])
@pytest.mark.parametrize("chunk", [1, 7])
def test_faulty_wave_at_small_size(chunk, shards):
    """config 3 at 300 members: kill at round 10, suspect timers fire from round 35 and dirty nearly every sender
    before it issues; three shards through the local port cover the remote checksum requests"""
    _, _, trace = oracle_trace("faulty300")
    assert trace[-1][2]["timers_fired"] > 0
    u = run_vs_oracle("faulty300", shards=shards, chunk=chunk)
    assert u["issue_snaps"] == 0, u


def test_small_dense_pool():
    """64 dense slots: the pool-bound path hashes the dirty senders before issue, the others stay pending, live"""
    u = run_vs_oracle("faulty333", dense_slots=64)
    assert u["issue_snaps"] == 0, u
