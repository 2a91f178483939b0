"""Incarnations past the checksum formatter's table through every entry point, on the MI355X engine against the CPU
oracle (tests/incarnation_scenarios.py has the scenarios, tests/test_incarnation_table_host.py what they reach on the
oracle alone; tests/test_dist_gpu.py runs the gossip scenario with one process per shard).

The checksum kernels clamp an incarnation step past their handle's table, so the host has to grow the table of every
handle whose rows can come to hold it before a round hashes them: the handle a raw write is made on, and the other
shards of its cluster, which the round's traffic carries the incarnation to. A handle that has not grown computes a
wrong checksum for those rows, and with it other full-sync decisions and another converged().

Every scenario runs on one handle and over the sharded split of its size (65 over 2, 130 over 3: uneven). Engine and
oracle are compared bit for bit after every round (test_engine_parity.run_parity: checksums, digests, targets, and
the counters at the end of each segment), the return values of every make_change and add_join_list, and at the end
every observer's row, dissemination buffer, timers, iterator and node statistics (test_fuzz.compare_final).
"""
import numpy as np
import pytest

import incarnation_scenarios as S
import swimsim
from oracle_ffi import OracleSim
from test_engine_parity import full_diff, run_parity
from test_fuzz import compare_final

pytestmark = pytest.mark.gpu

CASES = [(name, n) for name in S.NAMES for n in sorted(S.SPLITS)]
IDS = [f"{name}-{n}" for name, n in CASES]


def one_call(eng, ora, n, seg, label):
    """a segment that the engine runs as one step call of several rounds; compared after the call as run_parity does"""
    r0 = eng.round
    eng.step(seg["rounds"], seg["events"])
    for r in range(r0, r0 + seg["rounds"]):
        ora.step([e for e in seg["events"] if e[0] == r])
    et, ot = eng.last_targets(), ora.last_targets()
    assert (et == ot).all(), f"{label}: targets differ at {np.nonzero(et != ot)[0][:5]}"
    ec, oc = eng.checksums(), ora.checksums()
    if not (ec == oc).all() or eng.digest() != ora.digest():
        pytest.fail(f"{label}: divergence after the call of rounds {r0}..{r0 + seg['rounds'] - 1}: {full_diff(eng, ora, n)}")
    assert eng.counters() == ora.counters()


def run_scenario(eng, ora, sc, label):
    n = sc["n"]
    try:
        for i, seg in enumerate(sc["segments"]):
            erets = S.compared(seg["muts"], [S.apply(eng, op) for op in seg["muts"]])
            orets = S.compared(seg["muts"], [S.apply(ora, op) for op in seg["muts"]])
            assert erets == orets, f"{label}: return values of the writes before segment {i} differ"
            if seg.get("one_call"):
                one_call(eng, ora, n, seg, label)
            else:
                run_parity(eng, ora, n, seg["rounds"], seg["events"])
        assert eng.round == ora.round
        assert eng.converged() == ora.converged()
        compare_final(eng, ora, sc, label)
    except swimsim.SwimsimError as e:
        if "EHIP" in str(e):                                        # a device error: nothing more runs on this GPU
            pytest.exit(f"{label}: device error, the session ends here: {e}", returncode=3)
        raise


def single(sc):
    return swimsim.Cluster(sc["n"], **sc["engine_kw"])


def sharded(sc):
    return swimsim.ShardedCluster(sc["n"], S.SHARDED[sc["n"]], **sc["engine_kw"])


def check(make, sc, label):
    eng = make(sc)
    try:
        run_scenario(eng, OracleSim(sc["n"], **sc["oracle_kw"]), sc, label)
    finally:
        eng.close()


@pytest.mark.parametrize("name,n", CASES, ids=IDS)
def test_one_handle(name, n):
    check(single, S.scenario(name, n), f"{name}-{n} on one handle")


@pytest.mark.parametrize("name,n", CASES, ids=IDS)
def test_sharded(name, n):
    check(sharded, S.scenario(name, n), f"{name}-{n} over {S.SHARDED[n]} shards")


@pytest.mark.parametrize("make", [single, sharded], ids=["one_handle", "sharded"])
def test_default_table(make):
    """the gossip scenario at the bound of the default table of 65,536 entries (e = 65,535, 65,536 and 65,539)"""
    check(make, S.scenario("make_change", 65, "default"), f"make_change-65 under the default table, {make.__name__}")
