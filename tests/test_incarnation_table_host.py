"""The incarnation-table scenarios on the CPU oracle alone (tests/incarnation_scenarios.py): each can fail for the reason
it exists. No GPU.

For every scenario and split, after the first round that follows the first write:
  * at least one observer row of EVERY shard holds a hashed incarnation at or above the table's bound, although only
    observers of the first shard were written (the clock scenario steps one observer of every shard);
  * in the scenarios that spread by full sync, the oracle's full_syncs or rfs_done counter has moved, and in the gossip
    scenario change records have been sent;
  * for one such row of every shard, the checksum string with those incarnations replaced by the clamped one
    (t0 + (bound - 1) * period, what a handle with an ungrown table formats) hashes differently.
The second write (before round 4) puts new incarnations past the bound into rows of every shard as well.
"""
import numpy as np
import pytest

import incarnation_scenarios as S
from oracle_ffi import OracleSim, fingerprint32

SPLITS = [(n, shards) for n in sorted(S.SPLITS) for shards in S.SPLITS[n]]
CASES = [(name, n, shards, "small") for name in S.NAMES for n, shards in SPLITS]
CASES += [("make_change", n, shards, "default") for n, shards in SPLITS]


def past_bound(ora, sc):
    """bool [n, n]: observer o holds member m at a hashed status and an incarnation at or above the bound"""
    st, inc = ora.rows()
    return (st < S.TOMBSTONE) & (inc >= sc["t0_ms"] + sc["bound"] * sc["period_ms"])


def clamped_string(ora, sc, o):
    """observer o's checksum string as a handle whose table ends at the bound formats it"""
    _, inc = ora.row(o)
    clamp = b"%d;" % (sc["t0_ms"] + (sc["bound"] - 1) * sc["period_ms"])
    s = ora.checksum_string(o)
    for v in sorted({int(x) for x in inc[past_bound(ora, sc)[o]]}):
        s = s.replace(b"%d;" % v, clamp)
    return s


@pytest.mark.parametrize("name,n,shards,table", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_scenario_reaches_the_clamp_in_every_shard(name, n, shards, table):
    sc = S.scenario(name, n, table)
    ora = OracleSim(n, **sc["oracle_kw"])
    seen = {}

    def after_round(seg, k):
        if k != 1 or seg > 1:
            return
        hit = past_bound(ora, sc)
        seen[seg] = (hit.copy(), ora.counters())
        if seg:
            return
        for rank in range(shards):
            lo, hi = S.shard_range(n, shards, rank)
            rows = [o for o in range(lo, hi) if hit[o].any()]
            assert rows, f"no row of shard {rank} ({lo}..{hi - 1}) holds an incarnation past the bound after round 0"
            o = rows[-1]
            s = ora.checksum_string(o)
            assert fingerprint32(s) == ora.checksum(o)
            assert fingerprint32(clamped_string(ora, sc, o)) != ora.checksum(o), f"row {o}: the clamp does not show"
        if sc["table"] == "small":                                   # e = 40: the first 14-digit incarnation
            _, inc = ora.rows()
            assert {len(str(int(x))) for x in inc[hit]} == {13, 14} or name == "clock"

    rets = S.run_oracle(ora, sc, after_round)
    hit0, c0 = seen[0]
    print(f"{name} n={n} shards={shards}: rows past the bound after round 0: {int(hit0.any(axis=1).sum())}, "
          f"full_syncs {c0['full_syncs']} rfs_done {c0['rfs_done']} msg_changes {c0['msg_changes']}")
    if name in S.DENSE:
        assert c0["full_syncs"] + c0["rfs_done"] > 0
    if name == "make_change":
        assert c0["msg_changes"] > 0 and c0["full_syncs"] + c0["rfs_done"] == 0      # change records alone so far
        assert all(r == 1 for r in rets[0]), rets[0]                 # every status applied
    if name in S.RAW_WRITES:
        # the writers are all rows of the first shard, whichever split
        writers = {op[1] for seg in sc["segments"] for op in seg["muts"]}
        assert max(writers) < S.shard_range(n, S.SHARDED[n], 1)[0]
        # the second write's cells are new: rows of every shard hold more cells past the bound one round after it
        hit1, _ = seen[1]
        for rank in range(shards):
            lo, hi = S.shard_range(n, shards, rank)
            assert (hit1[lo:hi] & ~hit0[lo:hi]).any(), f"second write: nothing new in shard {rank}"
    else:
        c = ora.counters()
        _, p = S.clock_members(n)
        assert c["refutes"] > 0 and ora.member(p, p)[1] >= sc["t0_ms"] + 33 * sc["period_ms"]
        assert ora.round == 48 and ora.member(5, 5)[1] == 10**13


def test_rounds_and_sizes_are_what_the_gpu_tests_assume():
    for name in S.NAMES:
        sc = S.scenario(name, 65)
        assert sum(seg["rounds"] for seg in sc["segments"]) <= 30
        assert sc["engine_kw"]["max_rounds"] == 16 and "max_rounds" not in sc["oracle_kw"]
    assert S.TABLES["small"]["es"] == (15, 16, 17, 32, 40) and S.TABLES["default"]["es"] == (65535, 65536, 65539)
    assert S.T0_MS + 40 * S.PERIOD_MS == 10**13
    assert np.all([S.shard_range(n, s, s - 1)[1] == n for n in S.SPLITS for s in S.SPLITS[n]])
