"""The message pool where its sub-pools fill (pool_alloc_lane0): the move to the next sub-pool and a spilled
message's offset, the compare-and-swap retry, a fetch-add cursor past its sub-pool's end, the early response reservation
at a small sub-pool, and the refusal (SWIMSIM_ECAPACITY) once nothing fits. The automatic pool's sub-pools hold 16,384
records and more, which nothing the suite can afford fills, so every case sets message_pool_bytes: at the minimum the
smallest sub-pool holds N records (tests/pool_scenarios.py; the premises come from the oracle, tests/test_pool_host.py).

Every run steps one round per call against the oracle with test_engine_parity's comparison (targets, checksums, digests,
a full diff on divergence) and the counters, and must end in one of two ways: parity through the last round, or a step
refused with ECAPACITY after rounds that were all bit-exact. Which earlier round is refused is never asserted (the early
reservations ask for up to twice what the responses take); that a refusal comes no later than the round the oracle proves
it for is.

Measured on the MI355X (peak fill = the largest sum(min(cursor, sub)) / (64 * sub) over a run's rounds, from
Cluster.pool_usage() after each round; a refused round's fill is not read):
  SELFSTART, N = 128, 16 rounds   minimum x 1: refused in round 9 after a round at 0.833; x 2: parity, peak 0.654
                                  (round 11); x 4: parity, 0.327; x 16: parity, 0.125. The tight rung is x 2.
  the same over 2 / 3 shards      x 1: refused in round 10 (a shard at 0.897 / 0.719 the round before); x 1.5 (the
                                  tight rung per shard): parity, the fullest shard at 0.724 / 0.583; x 2: parity,
                                  0.543 / 0.438
  SELFSTART_FAIL, N = 512, x 1    refused in round 5 after a round at 0.816 (the requests alone exceed the pool in round
                                  6); step(8) refused; step(2) refused in its third call; x 16: parity, 0.244
  HEAVY, N = 256, x 1             rounds 0-3 exact at 0.171, 0.360, 0.570, 0.780; refused in round 4 (more than 64 heavy
                                  rows in round 6: their responses and ping-reqs are long too)
  SMALL, N = 512, x 1             parity; the largest cursor is 518 of 512 after round 0, as counted, and 603 after round 1
The refused rounds' own need was not measured (a refused handle is not read). By inference from the larger rungs the
refusals of SELFSTART are overflows and not the early reservation's doing: round 9 takes 0.573 of the x 2 pool, 1.15
minimum pools, and round 5 at N = 512 takes 0.131 of the x 16 pool, 2.1 minimum pools. Those cursor sums include the
larger rungs' own reservation slack (bounds of at most sub / 16: 16 records at x 2 against 8 at x 1), so the margin at
N = 128 is not exact; but a message needs one sub-pool with room for all of it, and with messages of up to N records in
sub-pools of N a need of about one pool cannot be placed either.
"""
import re

import numpy as np
import pytest

import swimsim
from oracle_ffi import OracleSim
from test_engine_parity import full_diff
from test_pool_host import heavy_profile, heavy_proven_round, proven_overflow_round, selfstart_requests
import pool_scenarios as S

pytestmark = pytest.mark.gpu

REFUSED = re.compile(r"ECAPACITY.*message pool overflow")


def same_state(eng, ora, n, r):
    """run_parity's comparison after round r, and the counters"""
    et, ot = eng.last_targets(), ora.last_targets()
    assert (et == ot).all(), f"round {r}: targets differ at {np.nonzero(et != ot)[0][:5]}"
    ec, oc = eng.checksums(), ora.checksums()
    if not (ec == oc).all() or eng.digest() != ora.digest():
        pytest.fail(f"round {r}: divergence: {full_diff(eng, ora, n)}")
    assert eng.counters() == ora.counters(), f"round {r}"


def fill_of(usage):
    """the filled share of one pool from (sub_records, cursors): a cursor past its sub-pool's end counts as full"""
    sub, cur = usage
    return float(np.minimum(cur, np.uint64(sub)).sum()) / (S.POOL_SUBS * sub)


def fills_of(eng):
    """per pool of the engine (one per shard)"""
    u = eng.pool_usage()
    return [fill_of(x) for x in u] if isinstance(u, list) else [fill_of(u)]


def drive(eng, ora, n, rounds, events=(), chunk=1):
    """`rounds` rounds, `chunk` per step call. Returns (refused, fills): refused = the first round of the call that
    ECAPACITY refused (None: parity through the last round), every call before it compared with the oracle; fills[i] =
    the pools' fills after call i (the last round of the call). A refused handle is not touched again."""
    fills = []
    for r in range(0, rounds, chunk):
        k = min(chunk, rounds - r)
        ev = [e for e in events if r <= e[0] < r + k]
        try:
            eng.step(k, ev)
        except swimsim.SwimsimError as e:
            assert REFUSED.search(str(e)), e
            return r, fills
        for q in range(r, r + k):
            ora.step([e for e in events if e[0] == q])
        same_state(eng, ora, n, r + k - 1)
        fills.append(fills_of(eng))
    return None, fills


def selfstart_pair(n, seeds, mult, shards=0):
    kw = dict(init="self", message_pool_bytes=S.pool_bytes(n, mult))
    eng = swimsim.ShardedCluster(n, shards, **kw) if shards else swimsim.Cluster(n, **kw)
    ora = OracleSim(n, init="self")
    S.seed_selfstart(n, seeds, eng, ora)
    return eng, ora


def run_selfstart(n, seeds, rounds, mult, shards=0, chunk=1):
    eng, ora = selfstart_pair(n, seeds, mult, shards)
    try:
        return drive(eng, ora, n, rounds, chunk=chunk)
    finally:
        eng.close()                              # (after a refusal: the only call the handle gets)


def run_heavy(rounds):
    n = S.HEAVY["n"]
    eng = swimsim.Cluster(n, message_pool_bytes=S.pool_bytes(n))
    ora = OracleSim(n)
    S.seed_heavy(eng, ora)
    try:
        return drive(eng, ora, n, rounds, S.HEAVY["events"])
    finally:
        eng.close()


def peak(fills):
    return max((max(f) for f in fills), default=0.0)


@pytest.fixture(scope="module")
def ladder():
    """ladder(mult): SELFSTART on the rung `mult`, run once per module and shared by the tests below"""
    runs = {}

    def run(mult):
        if mult not in runs:
            runs[mult] = run_selfstart(S.SELFSTART["n"], S.SELFSTART["seeds"], S.SELFSTART["rounds"], mult)
        return runs[mult]
    return run


def test_selfstart_ladder_is_exact_or_refused_and_monotone(ladder):
    n, rungs = S.SELFSTART["n"], S.SELFSTART["ladder"]
    reqs = selfstart_requests(n, S.SELFSTART["seeds"], S.SELFSTART["rounds"])
    out = {m: ladder(m) for m in rungs}
    for m in rungs:
        refused, fills = out[m]
        print(f"selfstart n={n} pool x{m}: refused in round {refused}, peak fill {peak(fills):.3f}, "
              f"per round {[round(f[0], 3) for f in fills]}")
        proven = proven_overflow_round(reqs, S.min_pool_records(n) * m)
        if proven is not None:
            assert refused is not None and refused <= proven, (m, refused, proven)
    passed = [out[m][0] is None for m in rungs]
    assert passed[-1], "the largest rung must run to full parity"
    assert passed == sorted(passed), f"refusals are not monotone in the pool size: {dict(zip(rungs, passed))}"


def test_heavy_rows_are_exact_until_refused_by_the_proven_round():
    proven = heavy_proven_round()
    refused, fills = run_heavy(S.HEAVY["rounds"])
    print(f"heavy rows {heavy_profile()}: refused in round {refused} (proven for round {proven}), "
          f"fill per round {[round(f[0], 3) for f in fills]}")
    assert refused is not None and refused <= proven
    # the rounds before the refusal are tight themselves: long messages, one or two to a sub-pool
    assert peak(fills) >= 0.5, fills


TIGHT_MULT = 2                                   # the smallest rung of SELFSTART that ran to parity on the MI355X


def test_tight_rung_runs_to_parity_at_half_a_pool_and_more(ladder):
    """minimum x 2 at N = 128: sub-pools of 256 records, messages of up to 128, peak fill 0.654 (round 11). With an
    allocator that tries only the sub-pool its wave starts at (a scratch build: the loop of pool_alloc_lane0 bounded by
    1 instead of POOL_SHARDS) this rung is refused, so the run depends on the move to the next sub-pool and on the
    offsets of the messages that moved; the fill is asserted so that the rung cannot quietly become a roomy one."""
    refused, fills = ladder(TIGHT_MULT)
    assert refused is None
    assert len(fills) == S.SELFSTART["rounds"]
    print(f"tight rung x{TIGHT_MULT}: peak fill {peak(fills):.3f}")
    assert peak(fills) >= 0.5


def test_small_allocations_pass_their_sub_pools_end_and_move_on():
    """SMALL: member 0's wave reserves one record per message, 511 of them, from one sub-pool of 512 that 7 requests
    share. The fetch-add path (allocations of at most sub / 256 records) leaves the cursor past the sub-pool's end and
    takes the next sub-pool; a scratch build that tries one sub-pool only refuses round 0."""
    n = S.SMALL["n"]
    eng, ora = selfstart_pair(n, S.SMALL["seeds"], 1)
    try:
        over = []
        for r in range(S.SMALL["rounds"]):
            eng.step(1)
            ora.step()
            same_state(eng, ora, n, r)
            sub, cur = eng.pool_usage()
            assert sub == n and cur.shape == (S.POOL_SUBS,)
            over.append(int(cur.max()))
        print(f"small: largest cursor per round {over} of {n}")
        assert over[0] > n, "no fetch-add cursor passed its sub-pool's end in round 0"
    finally:
        eng.close()


def test_multi_round_call_returns_the_refusal():
    """check_err runs once per step call, after its last round: the call that holds the overflowing round returns
    ECAPACITY whatever rounds follow it in the call, and every call before it is bit-exact"""
    c = S.SELFSTART_FAIL
    proven = proven_overflow_round(selfstart_requests(c["n"], c["seeds"], c["rounds"]), S.min_pool_records(c["n"]))
    refused, fills = run_selfstart(c["n"], c["seeds"], c["rounds"], 1, chunk=c["rounds"])
    assert refused == 0 and fills == []
    refused, fills = run_selfstart(c["n"], c["seeds"], c["rounds"], 1, chunk=2)
    assert refused is not None and refused <= proven and refused % 2 == 0
    assert len(fills) == refused // 2


def test_after_a_refusal_the_handle_closes_and_the_process_goes_on():
    c = S.SELFSTART_FAIL
    proven = proven_overflow_round(selfstart_requests(c["n"], c["seeds"], c["rounds"]), S.min_pool_records(c["n"]))
    eng, ora = selfstart_pair(c["n"], c["seeds"], 1)
    try:
        refused, _ = drive(eng, ora, c["n"], c["rounds"])
        assert refused is not None and refused <= proven
    finally:
        rc = swimsim.load_library().swimsim_destroy(eng.h)     # the refused handle's only call
        eng.h = None
    assert rc == 0
    # a new handle in the same process: the same scenario on the largest rung, to full parity
    refused, fills = run_selfstart(c["n"], c["seeds"], c["rounds"], S.SELFSTART["ladder"][-1])
    assert refused is None and len(fills) == c["rounds"]


SHARDED_RUNGS = (1, 1.5, 2, 16)                  # per shard; x 1.5 is the tight one (below), x 16 the largest of the ladder
SHARDED_TIGHT = 1.5


@pytest.mark.parametrize("shards", S.SELFSTART_SHARDS)
def test_sharded_pools_are_exact_or_refused(shards):
    """Every shard has a pool of its own, and the parcels another shard sends (requests to the seeds' rows on shard 0,
    their responses to every other shard) are allocated from it by k_x_unpack. The ladder per shard is minimum x 1,
    1.5, 2 and 16 with the same property as on one handle: exact or refused on every rung, monotone, the largest rung to
    parity. The tight rung is x 1.5, not the single handle's x 2, because a shard's pool takes only its own rows'
    share: at x 2 the fullest shard reaches 0.543 (2 shards) and 0.438 (3 shards), at x 1.5 0.724 and 0.583 (the other
    shards' peaks: 0.640; 0.485 and 0.448), and x 1.25 also ran to parity (0.868 / 0.700). The tight rung must run to
    parity with its fullest shard at half a pool and more; the one-sub-pool scratch build refuses it in round 1."""
    n, rounds = S.SELFSTART["n"], S.SELFSTART["rounds"]
    reqs = selfstart_requests(n, S.SELFSTART["seeds"], rounds)
    out = {}
    for mult in SHARDED_RUNGS:
        refused, fills = out[mult] = run_selfstart(n, S.SELFSTART["seeds"], rounds, mult, shards=shards)
        assert all(len(f) == shards for f in fills)
        per_shard = [round(max(f[k] for f in fills), 3) for k in range(shards)] if fills else []
        print(f"{shards} shards, pool x{mult} per shard: refused in round {refused}, peak fill per shard {per_shard}")
        assert proven_overflow_round(reqs, S.pool_records(n, mult)) is None   # (nothing proves a refusal here)
    passed = [out[m][0] is None for m in SHARDED_RUNGS]
    assert passed[-1], "the largest rung must run to full parity"
    assert passed == sorted(passed), f"refusals are not monotone in the pool size: {dict(zip(SHARDED_RUNGS, passed))}"
    refused, fills = out[SHARDED_TIGHT]
    assert refused is None and len(fills) == rounds
    assert peak(fills) >= 0.5, fills
