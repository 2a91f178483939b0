"""CPU side of the option tests: on the oracle alone, each scenario of tests/option_scenarios.py reaches the code it is
meant to reach. The GPU tests (tests/test_options.py) compare engine and oracle bit for bit on the same scenarios; a
later edit to a scenario that empties one of them fails here. Every guard is a condition; the figures in the comments
are what the oracle gives for the scenarios as they stand."""
import pytest

import option_scenarios as S
from oracle_ffi import OracleSim


def p_counters(k):
    return S.run_oracle(S.P_N, S.P_ROUNDS, S.P_EVENTS, ping_request_size=k).counters()


def test_partition_scenario_runs_every_ping_req_outcome_at_each_k():
    """scenario P: ping-reqs, helper errors, inconclusive runs and suspect declarations at every K, and more helper
    calls the larger K is (113 / 227 / 341 / 563 / 892 at K = 1 / 2 / 3 / 5 / 8; 177 ping-reqs at every K)"""
    calls = []
    for k in (1, 2, 3, 5, 8):
        c = p_counters(k)
        print(f"K={k}:", {x: c[x] for x in ("pingreqs", "helper_calls", "helper_errors", "inconclusive", "suspect_decl")})
        if k in S.P_KS:
            for name in ("pingreqs", "helper_errors", "inconclusive", "suspect_decl"):
                assert c[name] > 0, (k, name)
        calls.append(c["helper_calls"])
    assert all(a < b for a, b in zip(calls, calls[1:])), calls


def test_tiny_scenario_has_fewer_eligible_helpers_than_k():
    """scenario T at K = 8: at most 3 eligible helpers, so a run whose helpers all fail has fewer than K errors and
    declares a suspect (node.go:497); at K = 3 the same runs are inconclusive"""
    c8 = S.run_oracle(S.T_N, S.T_ROUNDS, S.T_EVENTS, ping_request_size=8).counters()
    c3 = S.run_oracle(S.T_N, S.T_ROUNDS, S.T_EVENTS, ping_request_size=3).counters()
    print("K=8:", c8, "K=3:", c3)
    assert c8["inconclusive"] == 0 and c8["suspect_decl"] == c8["pingreqs"] > 0          # 51 of 51
    assert c8["helper_errors"] > 0
    assert c3["inconclusive"] > 0                                                            # 6


@pytest.mark.parametrize("k", [3, 8])
def test_sparse_scenario_needs_the_helper_walk(k):
    """scenario S: in dozens of failed pings the 64 draws find too few helpers (most of them in rounds 0-1, when a
    row has about 4 pingable members out of 200)"""
    per_round = []
    walks, ora = S.walk_events(dict(ping_request_size=k), per_round=per_round)
    print(f"K={k}: {walks} walks, per round {per_round}")
    assert walks >= 50, walks
    assert ora.counters()["pingreqs"] >= walks


def test_sparse_scenario_fills_and_overflows_the_job_queues():
    """scenario S: a queue of 1 omits more reverse full syncs than it runs; a queue of 64 omits none and runs more
    than the default queue of 5 does (rfs_done 40 / 45 / 100 / 147, rfs_omitted 416 / 235 / 165 / 0 at 1 / 2 / 5 / 64)"""
    c = {}
    for jobs in (1, 2, 5, 64):
        ora = S.sparse_oracle(max_rfs_jobs=jobs)
        ora.run(S.S_ROUNDS, S.S_EVENTS)
        c[jobs] = ora.counters()
        print(f"jobs={jobs}: rfs_done {c[jobs]['rfs_done']} rfs_omitted {c[jobs]['rfs_omitted']}")
    assert c[1]["rfs_omitted"] > c[1]["rfs_done"] > 0
    assert c[2]["rfs_omitted"] > 0 and c[2]["rfs_done"] > 0
    assert c[64]["rfs_omitted"] == 0 and c[64]["rfs_done"] > c[5]["rfs_done"]
    # p_factor 1: a change leaves the buffer after one piggyback, so far more exchanges end in a full sync (596
    # against the default's, and 285 reverse full syncs)
    ora = S.sparse_oracle(p_factor=1)
    ora.run(S.S_ROUNDS, S.S_EVENTS)
    c1 = ora.counters()
    print(f"p_factor=1: full_syncs {c1['full_syncs']} (p_factor 15: {c[5]['full_syncs']}) rfs_done {c1['rfs_done']}")
    assert c1["full_syncs"] > c[5]["full_syncs"] and c1["rfs_done"] > c[5]["rfs_done"]


@pytest.mark.parametrize("case", S.M_CASES, ids=lambda c: f"n{c[0]}_pf{c[1]}")
def test_rumour_scenario_reaches_the_top_of_the_counter(case):
    """scenario M: the largest piggyback count in any buffer, sampled every round, is maxP - 1 (253 at maxP 254, 254
    at maxP 255: the largest value an accepted configuration can hold)"""
    n, pf, rounds = case
    seen = []
    ora = S.run_oracle(n, rounds, S.M_EVENTS, each_round=lambda ora, r: seen.append(S.largest_p(ora)), p_factor=pf)
    maxp = S.m_maxp(n, pf)
    assert maxp in (254, 255)
    live = [o for o in range(n) if o != 5]
    assert all(ora.maxp(o) == maxp for o in live)
    print(f"n={n} p_factor={pf}: maxP {maxp}, largest p {max(seen)}, first in round {seen.index(max(seen))}")
    assert max(seen) == maxp - 1


def test_create_refuses_over_limit_options_without_touching_device():
    """swimsim_create's option checks return before any device call: a p_factor whose largest maxP exceeds what the
    8-bit piggyback counter holds, and more than 8 helpers, are EINVAL with a message that names the option"""
    import swimsim
    for n, pf in ((130, 86), (12, 128), (9, 256), (1, 256), (130, 2**32 - 1)):
        assert pf * S.digits10(max(n - 1, 1)) > 255
        with pytest.raises(swimsim.SwimsimError, match=r"swimsim_create failed: EINVAL: p_factor"):
            swimsim.Cluster(n, p_factor=pf)
    with pytest.raises(swimsim.SwimsimError, match=r"swimsim_create failed: EINVAL: ping_request_size 9 .*limit of 8"):
        swimsim.Cluster(8, ping_request_size=9)
    with pytest.raises(swimsim.SwimsimError, match=r"swimsim_group_create failed: EINVAL: p_factor"):
        swimsim.ShardedCluster(130, 2, p_factor=86)
    with pytest.raises(swimsim.SwimsimError, match=r"EINVAL: ping_request_size"):
        swimsim.ShardedCluster(8, 2, ping_request_size=9)
    # a refusal without a text of its own does not repeat the previous one's
    with pytest.raises(swimsim.SwimsimError, match=r"swimsim_create failed: EINVAL$"):
        swimsim.Cluster(4, observer_range=(3, 2))


def test_seed_high_word_moves_the_first_round_targets():
    """the Philox key's high word is the seed's bits 32..63: the first round's ping targets at 64 members differ in
    most places between seeds that differ only there (63 and 62 of 64)"""
    def targets(seed):
        ora = OracleSim(64, seed=seed)
        ora.step()
        return ora.last_targets()
    for a, b in ((1, 1 | 1 << 32), (0, 1 << 32)):
        diff = int((targets(a) != targets(b)).sum())
        print(f"seeds {a:#x} / {b:#x}: {diff} of 64 targets differ")
        assert diff >= 32, diff
