"""The premises of the message-pool scenarios (tests/pool_scenarios.py), from the CPU oracle alone: what every round asks
of the pool, and hence in which round a minimum pool must overflow and on which rungs it need not. tests/test_pool.py
holds the engine to these; a drift of the workload generator or of the oracle fails here first, without a GPU."""
import functools

import numpy as np

from oracle_ffi import OracleSim
import pool_scenarios as S


@functools.lru_cache(maxsize=None)
def selfstart_requests(n, seeds, rounds):
    """records of the requests of rounds 0..rounds-1 of a self-only start"""
    ora = OracleSim(n, init="self")
    S.seed_selfstart(n, seeds, ora)
    out = []
    for _ in range(rounds):
        out.append(S.requests(ora))
        ora.step()
    return tuple(out)


def proven_overflow_round(reqs, pool_records):
    """the first round whose requests alone exceed the pool (None: no round does)"""
    return next((r for r, q in enumerate(reqs) if q > pool_records), None)


@functools.lru_cache(maxsize=None)
def heavy_profile():
    """rows with more than HEAVY_RECORDS buffer entries at the start of each of HEAVY's rounds"""
    ora = OracleSim(S.HEAVY["n"])
    S.seed_heavy(ora)
    out = []
    for r in range(S.HEAVY["rounds"]):
        out.append(S.heavy_rows(ora, S.HEAVY_RECORDS))
        ora.step([e for e in S.HEAVY["events"] if e[0] == r])
    return tuple(out)


def heavy_proven_round():
    """the first round with more than 64 allocations that each own a sub-pool: the requests of the heavy rows"""
    return next(r for r, k in enumerate(heavy_profile()) if k > S.POOL_SUBS)


def test_selfstart_512_outgrows_the_minimum_pool():
    reqs = selfstart_requests(S.SELFSTART_FAIL["n"], S.SELFSTART_FAIL["seeds"], S.SELFSTART_FAIL["rounds"])
    assert reqs == (1022, 1030, 3590, 6103, 9970, 21072, 32842, 43176)
    pool = S.min_pool_records(S.SELFSTART_FAIL["n"])
    assert pool == 32768
    proven = proven_overflow_round(reqs, pool)
    assert proven is not None and proven <= 7 and reqs[7] > pool
    assert proven < S.SELFSTART_FAIL["rounds"]


def test_selfstart_128_requests_fit_every_rung():
    n = S.SELFSTART["n"]
    reqs = selfstart_requests(n, S.SELFSTART["seeds"], S.SELFSTART["rounds"])
    assert max(reqs) == 5624 and int(np.argmax(reqs)) == 11
    for mult in S.SELFSTART["ladder"]:
        assert proven_overflow_round(reqs, S.min_pool_records(n) * mult) is None
    assert S.SELFSTART["ladder"] == (1, 2, 4, 16)


def test_heavy_rows_outnumber_the_sub_pools():
    assert S.pool_bytes(S.HEAVY["n"]) // S.RECORD_BYTES // S.POOL_SUBS == 2 * S.HEAVY_RECORDS
    prof = heavy_profile()
    assert prof[0] == len(S.HEAVY["observers"])
    proven = heavy_proven_round()
    assert prof[proven] > S.POOL_SUBS and all(k <= S.POOL_SUBS for k in prof[:proven])
    assert sum(8 <= k <= 32 for k in prof[:proven]) >= 3, prof
    assert proven == S.HEAVY["rounds"] - 1, prof


def test_small_reservations_overflow_one_sub_pool():
    """round 0 of SMALL: every other member pings member 0 with one record, and member 0's buffer is empty, so its wave
    reserves one record per message from the sub-pool of wave 0; the requests of senders 64, 128, ... share it"""
    n = S.SMALL["n"]
    sub = S.min_pool_records(n) // S.POOL_SUBS
    ora = OracleSim(n, init="self")
    S.seed_selfstart(n, S.SMALL["seeds"], ora)
    cc = [ora.changes_count(o) for o in range(n)]
    assert cc[0] == 0 and all(c == 1 for c in cc[1:]) and 1 <= sub // 256
    ora.step()
    t = ora.last_targets()
    assert (t[1:] == 0).all() and t[0] < 0
    asked = (n - 1) + sum(cc[o] for o in range(0, n, S.POOL_SUBS))
    assert asked == 518 and asked > sub
