"""What the shapes of tests/resp_echo_cases.py reach, shown on the CPU oracle alone (no GPU): the premises of
tests/test_resp_echo.py, which runs the same shapes on the engine with echoed response records left out and written.

An echo needs a sender and a receiver that agree on a buffered member. The strongest form, every live row buffering all
k killed members at once, is reached within the 14 rounds by five of the nine cascades (resp_echo_cases.ALL_ROWS_FULL);
the oracle does not reach it at (257, 64) (the last record arrives after round 13) and at n = 1,100 (844 live nodes
need about six rounds to have pinged each of the 256 to 300 killed ones once, and a record then needs more than the
rounds left to reach every row). Every cascade has ping pairs that agree on a buffered member from the third round
after the kill on, which is what an echo needs; both are asserted below.
"""
import functools

import pytest

import fuzz_scenarios as F
import resp_echo_cases as R
from oracle_ffi import OracleSim


def snapshot(ora):
    return ora.rows(), [ora.dis_entries(o) for o in range(ora.n)]


@functools.lru_cache(maxsize=None)
def cascade_trace(n, k):
    """(rounds in which every live row buffers all k killed members, echo pairs per round, the oracle's counters)"""
    ora = OracleSim(n, **R.CASCADE_OPTS)
    ev, ks = R.cascade_events(n, k), R.killed(n, k)
    assert len(set(ks)) == k and 0 not in ks and max(ks) < n
    full, pairs, mixed = [], [], 0
    for r in range(R.ROUNDS):
        rows, dis = snapshot(ora)
        live = [o for o in range(n) if ora.live(o)]
        # killed members on whose status the live rows differ (suspect here, faulty there) before the round
        mixed = max(mixed, sum(1 for m in ks if len({int(rows[0][o][m]) for o in live}) > 1))
        ora.step([e for e in ev if e[0] == r])
        pairs.append(R.echo_pairs(ora, rows, dis))
        if R.all_rows_hold(ora, ks):
            full.append(r)
    return full, pairs, dict(ora.counters(), mixed=mixed)


@pytest.mark.parametrize("n,k", R.CASCADES, ids=[f"{n}-{k}" for n, k in R.CASCADES])
def test_cascade_has_ping_pairs_that_agree_on_a_buffered_member(n, k):
    full, pairs, ctr = cascade_trace(n, k)
    print(f"cascade {n}-{k}: all rows full in rounds {full}; agreeing ping pairs per round {pairs}")
    assert sum(pairs[:R.KILL_ROUND + 1]) == 0                       # nothing is buffered before the kill is noticed
    assert all(p > 0 for p in pairs[R.KILL_ROUND + 3:]), pairs
    assert pairs[-1] > (n - k) // 2, pairs                          # most live senders by the last round
    assert ctr["helper_calls"] > 0 and ctr["suspect_decl"] >= k
    # the faulty wave runs inside the 14 rounds: timers fired, and in some round live rows differed on the status of a
    # killed member (a receiver then holds a higher pair than the one it is sent: not an echo)
    assert ctr["timers_fired"] > 0 and ctr["mixed"] > 0, ctr


@pytest.mark.parametrize("n,k", R.ALL_ROWS_FULL, ids=[f"{n}-{k}" for n, k in R.ALL_ROWS_FULL])
def test_cascade_rounds_in_which_all_live_rows_buffer_all_killed_members(n, k):
    full, _, _ = cascade_trace(n, k)
    assert full and full[-1] == R.ROUNDS - 1, full


@pytest.mark.parametrize("name", sorted(R.WALKS))
def test_walk_shapes(name):
    n, ev, tuning, opts = R.WALKS[name]
    ora = OracleSim(n, **opts)
    most = 0
    for r in range(R.ROUNDS):
        ora.step([e for e in ev if e[0] == r])
        cnt = [ora.changes_count(o) for o in range(n) if ora.live(o)]
        most = max(most, max(cnt))
    ctr = ora.counters()
    np_ = (n + 63) // 64 * 64                                       # the engine's padded row
    if name.startswith(("mixed", "churn")):
        assert most > tuning["hot_slots"]                           # more buffered members than hot slots: cold entries
    if name.startswith("churn"):
        assert 4 * most > np_ and ctr["refutes"] + ctr["applied"] > 0   # the streaming walk's threshold
    if name == "mixed-257":
        assert 4 * most <= np_                                      # the presence-bitmap walk throughout
    if name.startswith("pingreq"):
        assert ctr["helper_calls"] > 2 * ctr["pingreqs"] > 0, ctr   # several helpers per sender
    assert ctr["helper_calls"] > 0, ctr


@functools.lru_cache(maxsize=None)
def fuzz_trace(n, seed):
    c = F.case(n, seed)
    return R.fuzz_premises(OracleSim(n, init=c["init"], **c["options"]), c)


@pytest.mark.parametrize("n,seed", R.EVICTED_BUFFERED, ids=[f"{n}-{s}" for n, s in R.EVICTED_BUFFERED])
def test_an_evicted_member_is_still_buffered(n, seed):
    """its record reads (tombstone, inc) and comes from an UNKNOWN row: the first exclusion"""
    evicted, _ = fuzz_trace(n, seed)
    assert len(evicted) >= 3, evicted


@pytest.mark.parametrize("n,seed", R.STEPPED_BACK_REFUTE, ids=[f"{n}-{s}" for n, s in R.STEPPED_BACK_REFUTE])
def test_a_node_on_a_stepped_back_clock_refutes_in_a_round_in_which_it_pinged(n, seed):
    """the refute writes now(o), which a stepped-back clock may put below what o sent: the second exclusion"""
    _, refutes = fuzz_trace(n, seed)
    assert refutes, refutes


def test_the_exclusion_cases_are_committed_fuzz_cases():
    assert set(R.EXCLUSIONS) <= set(F.CASES)
