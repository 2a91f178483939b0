"""Every swim.Options knob that steers the round kernels, off its default, engine against CPU oracle, bit for bit:
ping_request_size (K), max_reverse_full_sync_jobs, p_factor and the 64-bit seed. Every other parity test of the
suite runs K = 3, 5 jobs, pFactor 15 and seed 1.

K is the stride of the ping-req phases' buffers (the helper table, the helper responses, the inbox value
observer * K + slot that seven kernels and the cross-shard parcels decode), the job limit sizes the reverse-full-sync
queues, pFactor sets maxP, which the 8-bit piggyback counter of a dissemination cell must hold, and the seed's high
word is half of the Philox key. The scenarios are in tests/option_scenarios.py; tests/test_options_host.py proves on
the oracle alone that each of them reaches the code it is meant to reach.
"""
from contextlib import closing

import pytest

import option_scenarios as S
import swimsim
from swimsim import workloads as W
from test_engine_parity import make_pair, run_parity
from test_sharded_parity import make_sharded

pytestmark = pytest.mark.gpu


# ---- 1. K in the ping-req phases -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", S.P_KS)
def test_partition_scenario_at_k(k):
    eng, ora = make_pair(S.P_N, ping_request_size=k)
    with closing(eng):
        run_parity(eng, ora, S.P_N, S.P_ROUNDS, S.P_EVENTS)
        c = eng.counters()
        assert c["helper_errors"] > 0 and c["inconclusive"] > 0 and c["suspect_decl"] > 0, c


# ---- 2. the cross-shard ping-req parcels at a K that is not 3 --------------------------------------------------------
@pytest.mark.parametrize("k,shards", [(8, 3), (5, 2)])
def test_partition_scenario_sharded(k, shards):
    eng, ora = make_sharded(S.P_N, shards, ping_request_size=k)
    with closing(eng):
        run_parity(eng, ora, S.P_N, S.P_ROUNDS, S.P_EVENTS)
        assert all(i["exchanges"] > 0 for i in eng.shard_info())


# ---- 3. fewer eligible helpers than K --------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 3])
def test_tiny_scenario_fewer_helpers_than_k(k):
    """six members, two dead, one cut off: at K = 8 a run whose helpers all fail has fewer than K errors and declares a
    suspect (node.go:497 compares with PingRequestSize, not with the helpers found)"""
    eng, ora = make_pair(S.T_N, ping_request_size=k)
    with closing(eng):
        run_parity(eng, ora, S.T_N, S.T_ROUNDS, S.T_EVENTS)
        ec, oc = eng.counters(), ora.counters()
        assert ec["inconclusive"] == oc["inconclusive"] and ec["suspect_decl"] == oc["suspect_decl"]
        if k == 8:
            assert ec["inconclusive"] == 0 and ec["suspect_decl"] == ec["pingreqs"] > 0
        else:
            assert ec["inconclusive"] > 0


# ---- 4. sparse rows: the helper walk, the job queues, pFactor 1 ------------------------------------------------------
def run_sparse(eng, ora):
    got = S.seed_sparse([eng, ora])
    assert got[0] == got[1]
    run_parity(eng, ora, S.S_N, S.S_ROUNDS, S.S_EVENTS)
    c = ora.counters()
    assert c["pingreqs"] > 0 and c["full_syncs"] > 0 and c["rfs_done"] > 0
    return c


@pytest.mark.parametrize("k,jobs,pf", [(3, 5, 15), (8, 64, 15), (1, 1, 15), (8, 2, 1)])
def test_sparse_scenario(k, jobs, pf):
    """200 nodes that know members 0..3 only: the 64 helper draws run dry and k_helpers walks the row; queues of 1,
    2, 5 and 64 reverse full syncs"""
    eng, ora = make_pair(S.S_N, init="self", ping_request_size=k, max_rfs_jobs=jobs, p_factor=pf)
    with closing(eng):
        c = run_sparse(eng, ora)
        assert (c["rfs_omitted"] == 0) == (jobs == 64), c


def test_sparse_scenario_sharded():
    eng, ora = make_sharded(S.S_N, 3, init="self", ping_request_size=8, max_rfs_jobs=64)
    with closing(eng):
        run_sparse(eng, ora)
        assert all(i["exchanges"] > 0 for i in eng.shard_info())


# ---- 5. the seed's high word ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1 | 1 << 32, 1 << 32, 0, 2**64 - 1], ids=hex)
def test_seed(seed):
    wl = W.config2(n=256, rounds=30)
    eng, ora = make_pair(wl.n, seed=seed)
    with closing(eng):
        run_parity(eng, ora, wl.n, wl.rounds, wl.events)


# ---- 6. the piggyback counter at the top of its 8 bits ---------------------------------------------------------------
@pytest.mark.parametrize("case", S.M_CASES[:2], ids=lambda c: f"n{c[0]}_pf{c[1]}")
def test_rumour_scenario_counter_peak(case):
    """maxP = 254 and 255, the largest the engine accepts: the rumour's count climbs to maxP - 1 (0xFE at maxP 255;
    0xFF is "no entry") in rounds 146 .. 162 and the entry then leaves, all in parity. Rounds 140 .. 169 are compared
    one by one, and in each of them the buffers of observer 0 and of the observer with the largest count are
    compared entry by entry."""
    n, pf, rounds = case
    maxp = S.m_maxp(n, pf)
    eng, ora = make_pair(n, p_factor=pf)
    with closing(eng):
        assert eng.node(0).disseminator.MaxP() == ora.maxp(0)
        run_parity(eng, ora, n, 140, S.M_EVENTS, check_every=10)
        assert ora.maxp(0) == maxp
        peak = -1
        for _ in range(30):
            run_parity(eng, ora, n, 1, S.M_EVENTS)
            top = {o: max((e[0] for e in ora.dis_entries(o).values()), default=-1) for o in range(n)}
            holder = max(top, key=top.get)
            for o in {0, holder}:
                got = eng.changes(o)
                assert got == ora.dis_entries(o), f"round {eng.round - 1}, observer {o}"
                peak = max([peak] + [e[0] for e in got.values()])
        assert peak == maxp - 1, peak                         # read from the engine's cells
        run_parity(eng, ora, n, rounds - 170, S.M_EVENTS, check_every=10)
        assert not ora.dis_entries(0) and not eng.changes(0)  # the rumour has left


# ---- 7. the limits: refused, never a silently wrong result -----------------------------------------------------------
@pytest.mark.parametrize("make", [swimsim.Cluster, lambda n, **kw: swimsim.ShardedCluster(n, 2, **kw)],
                         ids=["cluster", "sharded"])
def test_limits_are_refused_with_a_message(make):
    with pytest.raises(swimsim.SwimsimError, match=r"EINVAL.*p_factor"):
        make(130, p_factor=86)                                # maxP = 86 * 3 = 258
    with pytest.raises(swimsim.SwimsimError, match=r"EINVAL.*p_factor"):
        make(12, p_factor=128)                                # maxP = 128 * 2 = 256
    with pytest.raises(swimsim.SwimsimError, match=r"EINVAL.*ping_request_size.*limit of 8"):
        make(8, ping_request_size=9)


def test_largest_accepted_options_run():
    """maxP = 255 at one digit (9 members, pFactor 255) steps in parity; K = 8 is accepted"""
    eng, ora = make_pair(9, p_factor=255)
    with closing(eng):
        run_parity(eng, ora, 9, 3, [(0, W.EV_KILL, 5, 0)])
        assert eng.node(0).disseminator.MaxP() == ora.maxp(0) == 255
    with closing(swimsim.Cluster(8, ping_request_size=8)) as eng:
        eng.step(1)
