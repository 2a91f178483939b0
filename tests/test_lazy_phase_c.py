"""Lazy phase C (swimsim_tuning.cs_defer): a round inside a multi-round step call may leave its dirty
rows unhashed for a later round of the same call. Nothing a caller can read changes: every run here is compared with the
CPU oracle at every call boundary, where the read-backs are defined: checksums, the three state digests (rows,
dissemination, timers), the protocol counters (full_syncs among them) and the last ping targets.

cs_defer 2 (tests only) skips whenever a round follows in the call, whatever the row count, so sizes of a few hundred
members reach every path a carried row takes: pending-live senders in every round, deferred decisions over carried
receivers and senders (direct compare, undo log, late rebuild, hash of a rebuilt sender), heal pings inside a call, and
the checksum requests between shards. cs_defer 0 is the engine before the change; 1 (default) is the policy.
"""
import functools

import numpy as np
import pytest

from oracle_ffi import OracleSim
import swimsim
from swimsim import workloads as W

pytestmark = pytest.mark.gpu

NO_DIRECT, NO_REP, NO_UNDO, UNDO_CAP2 = 1, 2, 4, 8   # swimsim_tuning.defer_test


def raw_writes(n=512, rounds=4):
    """a converged cluster; before round 0 every receiver's row gets one raw write (member o + 1 suspect at a newer
    incarnation, each row another member): no row has anything to disseminate, every ping is empty, every row differs
    from its pinger's, so every decision needs both checksums and ends as a full sync"""
    wl = W.Workload(f"raw_writes_n{n}", n, rounds, [], "one raw row write per node, then empty pings")
    return wl, {0: [("set_member", o, (o + 1) % n, swimsim.SUSPECT, swimsim.T0_MS + 200) for o in range(n)]}


WORKLOADS = {
    "cascade1024": lambda: W.config3(n=1024, rounds=45, kill_round=3),
    "cascade2048": lambda: W.config3(n=2048, rounds=45, kill_round=3),
    "faulty300": lambda: W.config3(n=300, rounds=63, kill_round=10),           # (tests/test_lazy_issue.py's)
    "cascade1000": lambda: W.config3(n=1000, rounds=45, kill_round=5),         # (tests/test_lazy_issue.py's)
    "raw_writes": raw_writes,
    "heal512": lambda: W.config4(n=512, rounds=44, split_until=30, heals=(30, 38)),
    "selfstart512": lambda: W.selfstart(n=512, seeds=2, rounds=12),
}


@functools.lru_cache(maxsize=None)
def oracle_trace(key):
    """the workload and the oracle's record of it after every round: (checksums, digests, counters, last targets).
    Computed once per workload and shared; nothing changes it."""
    wl = WORKLOADS[key]()
    wl, acts = wl if isinstance(wl, tuple) else (wl, {})
    ora = OracleSim(wl.n, init=wl.init)
    for o in range(wl.n):
        for m in wl.seed_members:
            if m != o:
                ora.make_change(o, m, swimsim.T0_MS, 0)
    trace = []
    for r in range(wl.rounds):
        for (f, *args) in acts.get(r, ()):
            getattr(ora, f)(*args)
        ora.step(wl.events_for(r))
        cs = ora.checksums().copy()
        cs.setflags(write=False)
        tg = ora.last_targets().copy()
        tg.setflags(write=False)
        trace.append((cs, ora.digest(), ora.counters(), tg))
    return wl, acts, tuple(trace)


def compare(eng, trace, r, tag):
    """the read-backs after the call that ended with round r against the oracle's record of round r"""
    cs, digest, counters, targets = trace[r]
    ec = eng.counters()
    fs = {f: (ec[f], counters[f]) for f in ("full_syncs", "full_syncs_pingreq")}
    assert ec == counters, f"{tag} round {r}: counters differ, full syncs {fs}"
    bad = np.nonzero(eng.checksums() != cs)[0]
    assert len(bad) == 0, f"{tag} round {r}: {len(bad)} checksums differ, rows {bad[:5]}"
    ed = eng.digest()
    assert ed == digest, f"{tag} round {r}: digests (rows, dissemination, timers) {ed} != {digest}"
    assert np.array_equal(eng.last_targets(), targets), f"{tag} round {r}: last targets differ"


def run_vs_oracle(key, chunks, *, shards=0, **tuning):
    """one engine run of workload `key`, stepped in calls of chunks[i % len(chunks)] rounds (a call never crosses a
    round with scripted writes) and compared with the oracle after every call; returns kernel_units()"""
    wl, acts, trace = oracle_trace(key)
    tag = f"{key} chunks {chunks} shards {shards} {tuning}"
    if shards:
        eng = swimsim.ShardedCluster(wl.n, shards, init=wl.init, tuning=tuning or None)
    else:
        eng = swimsim.Cluster(wl.n, init=wl.init, tuning=tuning or None)
    try:
        for o in range(wl.n):
            for m in wl.seed_members:
                if m != o:
                    eng.make_change(o, m, swimsim.T0_MS, swimsim.ALIVE)
        r, i = 0, 0
        while r < wl.rounds:
            k = min(chunks[i % len(chunks)], wl.rounds - r)
            nxt = min((a for a in acts if a > r), default=wl.rounds)
            k = min(k, nxt - r)
            i += 1
            for (f, *args) in acts.get(r, ()):
                getattr(eng, f)(*args)
            eng.step(k, [e for e in wl.events if r <= e[0] < r + k])
            r += k
            compare(eng, trace, r - 1, tag)
        u = eng.kernel_units()
        print(tag, {k: int(v) for k, v in u.items() if k.startswith(("defer", "lazy", "issue_", "cs_"))})
        return u
    finally:
        eng.close()


# ---- 1. the cascade, both waves and the gap between them ----
@pytest.mark.parametrize("shards", [0, 3])
@pytest.mark.parametrize("chunk", [2, 3, 7])
def test_cascade_forced_skips(chunk, shards):
    u = run_vs_oracle("cascade1024", (chunk,), shards=shards, cs_defer=2)
    assert u["cs_skipped_rounds"] > 0 and u["cs_carried_rows"] > 0, u
    assert u["cs_forced"] == 0, u


@pytest.mark.parametrize("shards", [0, 3])
def test_cascade_every_round_hashed(shards):
    """cs_defer 0, one round per call: the same arrays at the same rounds (the oracle's), and nothing skipped"""
    u = run_vs_oracle("cascade1024", (1,), shards=shards, cs_defer=0)
    assert u["cs_skipped_rounds"] == 0 and u["cs_carried_rows"] == 0 and u["cs_forced"] == 0, u


def test_cs_defer_off_never_skips_in_long_calls():
    u = run_vs_oracle("cascade1024", (7,), cs_defer=0, cs_async_rows=64)
    assert u["cs_skipped_rounds"] == 0 and u["cs_carried_rows"] == 0 and u["cs_forced"] == 0, u


# ---- 2. the faulty wave at 300 members: decisions over carried rows through every way of settling them ----
@pytest.mark.parametrize("defer_test", [0, NO_DIRECT, NO_REP, NO_UNDO, UNDO_CAP2, NO_DIRECT | NO_REP | NO_UNDO | UNDO_CAP2])
def test_faulty_wave_forced_paths(defer_test):
    """Calls of 5 rounds: the first round of a call issues from hashed rows, the other four from carried ones, so their
    senders are pending, live. A pending-live sender's decision is compared against its row with the undo log undone
    (counted defer_eq; no test bit switches it off). Three members die here, so no row logs a third change in one
    phase and the 2-entry log (bit 8) never overflows: the 1,000-member cascade below forces that."""
    kw = dict(defer_test=defer_test) if defer_test else {}
    u = run_vs_oracle("faulty300", (5,), cs_defer=2, **kw)
    assert u["cs_skipped_rounds"] > 0 and u["cs_carried_rows"] > 0, u
    assert u["issue_snaps"] == 0 and u["defer"] > 0 and u["defer_eq"] > 0, u
    if defer_test & NO_UNDO:
        assert u["defer_undo"] == 0, u


@pytest.mark.parametrize("defer_test", [UNDO_CAP2, NO_DIRECT | NO_REP | NO_UNDO | UNDO_CAP2])
def test_late_rebuilds_of_carried_senders(defer_test):
    """tests/test_lazy_issue.py's cascade (1,000 members, 10 die): with a log of 2 entries a pending-live sender that
    applies a third change in a phase is rebuilt by its receive wave (lazy_late). Every sender of a call's later rounds
    is pending, live, and in both waves a row applies up to 10 changes per phase."""
    u = run_vs_oracle("cascade1000", (5,), cs_defer=2, defer_test=defer_test)
    assert u["cs_skipped_rounds"] > 0 and u["cs_carried_rows"] > 0, u
    assert u["issue_snaps"] == 0 and u["defer_eq"] > 0 and u["lazy_late"] > 0, u


def test_faulty_wave_undo_log_and_rebuilt_sender():
    """direct compare and representatives off (bits 1 | 2): decisions whose sender was clean at issue go through the
    undo log (defer_undo); with the undo log off as well (1 | 2 | 4) the same decisions hash the receiver's snapshot.
    Decisions whose rows differ need the pending-live sender's checksum: its issue-time row is rebuilt and hashed
    (lazy_mat); the raw-writes workload below makes every decision such a one."""
    u = run_vs_oracle("faulty300", (5,), cs_defer=2, defer_test=NO_DIRECT | NO_REP)
    assert u["cs_skipped_rounds"] > 0 and u["defer_eq"] > 0 and u["defer_undo"] > 0, u


# ---- 3. decisions against unhashed rows ----
@pytest.mark.parametrize("defer_test", [0, UNDO_CAP2])
def test_decisions_against_unhashed_rows(defer_test):
    """every row differs from its pinger's and nobody has anything to send: every ping's decision needs the sender's
    and the receiver's checksums while both rows are dirty and unhashed (raw writes before the call). The senders are
    rebuilt and hashed (lazy_mat), the rounds after carry the rows the full syncs wrote, and the full syncs are the
    oracle's (compare() checks every counter)."""
    wl, _, trace = oracle_trace("raw_writes")
    assert trace[0][2]["full_syncs"] >= wl.n // 2, trace[0][2]
    kw = dict(defer_test=defer_test) if defer_test else {}
    u = run_vs_oracle("raw_writes", (4,), cs_defer=2, **kw)
    assert u["cs_skipped_rounds"] > 0 and u["cs_carried_rows"] > 0, u
    assert u["defer"] > 0 and u["lazy_mat"] > 0 and u["defer_fs"] > 0, u


def test_decisions_against_carried_rows_in_every_round():
    """the raw writes' decisions all fall into the call's first round (the full syncs give every sender something to
    send). A self-only start keeps deciding: every round of it ends hundreds of empty-list pings as full syncs, here
    with every row carried from the round before"""
    _, _, trace = oracle_trace("selfstart512")
    assert trace[3][2]["full_syncs"] > trace[1][2]["full_syncs"] > trace[0][2]["full_syncs"] > 0
    u = run_vs_oracle("selfstart512", (4,), cs_defer=2)
    assert u["cs_skipped_rounds"] > 0 and u["cs_carried_rows"] > 0, u
    assert u["defer"] > 0 and u["lazy_late"] + u["lazy_mat"] > 0 and u["defer_fs"] > 0, u


# ---- 4. heal inside a call ----
@pytest.mark.parametrize("shards", [0, 3])
def test_heal_inside_a_call(shards):
    """partition for 30 rounds (the other half is faulty by then), heals at rounds 30 and 38; the calls of 9 rounds
    that hold them (27-35, 36-43) carry rows into the heal round: do_heal reads the healer's row and ping_with hashes
    the one sender it needs"""
    wl, _, trace = oracle_trace("heal512")
    assert trace[-1][2]["heal_attempts"] > 0, trace[-1][2]
    u = run_vs_oracle("heal512", (9,), shards=shards, cs_defer=2)
    assert u["cs_skipped_rounds"] > 0 and u["cs_carried_rows"] > 0, u


# ---- 5. the default policy and its valve ----
def test_default_policy_skips_inside_the_waves_only():
    """2,048 members, launches of more than 64 rows count as wide: one call over the whole cascade skips rounds of the
    two waves and hashes the others (the quiet rounds before the kill, the rounds after each wave, the last one)"""
    wl, _, _ = oracle_trace("cascade2048")
    u = run_vs_oracle("cascade2048", (wl.rounds,), cs_async_rows=64)
    assert 0 < u["cs_skipped_rounds"] < wl.rounds, u
    assert u["cs_carried_rows"] > 64 * u["cs_skipped_rounds"], u


def test_valve_on_a_self_only_start():
    """every round of a self-only start defers many decisions (every sender is dirty, most rows differ): the policy
    must not carry rows into them"""
    wl, _, _ = oracle_trace("selfstart512")
    u = run_vs_oracle("selfstart512", (wl.rounds,), cs_async_rows=64)
    assert u["cs_forced"] > 0 or u["cs_skipped_rounds"] == 0, u


# ---- 6. per-round callers ----
def test_one_round_per_call_is_unchanged():
    u = run_vs_oracle("cascade1024", (1,))
    assert u["cs_skipped_rounds"] == 0 and u["cs_carried_rows"] == 0 and u["cs_forced"] == 0, u
    u = run_vs_oracle("cascade1024", (1,), cs_async_rows=64)
    assert u["cs_skipped_rounds"] == 0 and u["cs_carried_rows"] == 0 and u["cs_forced"] == 0, u
