"""What the shapes of tests/slot_bump_cases.py reach, shown on the CPU oracle alone (no GPU): the premises of
tests/test_slot_bump.py, which runs the same shapes on the engine with the bump taken from the sender's bitmap of sent
slots and from its records.
"""
import functools

import pytest

import fuzz_scenarios as F
import slot_bump_cases as S
from oracle_ffi import OracleSim


@functools.lru_cache(maxsize=None)
def pf1_trace(name):
    """(deletions at maxP seen, the largest maxP of a live row, the oracle's counters): a deletion at maxP is a live row
    whose buffer loses a member in a round in which none of the row's status words or incarnations changes (an entry
    leaves a buffer only at maxP, or when a change for its member applies, which writes the row)"""
    n, ev, _, opts = S.PF1[name] if name in S.PF1 else S.PINGREQ[name]
    ora = OracleSim(n, **opts)
    deletions, maxp = 0, 0
    for r in range(S.ROUNDS):
        live = [o for o in range(n) if ora.live(o)]
        before = {o: (set(ora.dis_entries(o)), ora.row(o)) for o in live}
        ora.step([e for e in ev if e[0] == r])
        for o in live:
            if not ora.live(o):
                continue
            buf, (st, inc) = before[o]
            st2, inc2 = ora.row(o)
            if (st == st2).all() and (inc == inc2).all() and buf - set(ora.dis_entries(o)):
                deletions += 1
            maxp = max(maxp, ora.maxp(o))
    return deletions, maxp, ora.counters()


@pytest.mark.parametrize("name", sorted(S.PF1))
def test_p_factor_1_cascades_delete_entries_at_maxp(name):
    deletions, maxp, ctr = pf1_trace(name)
    print(f"{name}: {deletions} row-rounds with a deletion at maxP, maxP {maxp}, counters {ctr}")
    assert maxp == 3                                                # 1 x digits10(members)
    assert deletions > 0
    assert ctr["pings_ok"] > 0 and ctr["suspect_decl"] > 0


def test_p_factor_1_mixed_shapes_hold_more_members_than_hot_slots():
    for name in ("pf1-mixed-130", "pf1-mixed-257"):
        n, ev, tuning, opts = S.PF1[name]
        ora = OracleSim(n, **opts)
        seen = set()
        for r in range(S.ROUNDS):
            ora.step([e for e in ev if e[0] == r])
            for o in range(n):
                if ora.live(o):
                    seen |= set(ora.dis_entries(o))
        assert len(seen) > tuning["hot_slots"], (name, len(seen))  # some buffered member finds no slot: cold entries


@pytest.mark.parametrize("name", sorted(S.PINGREQ))
def test_ping_req_shapes_have_helper_errors(name):
    """a failed helper is what makes the sender bump in phase Q3 (ping_request_sender.go:105-106)"""
    _, _, ctr = pf1_trace(name)
    assert ctr["helper_errors"] > 0 and ctr["helper_calls"] > 2 * ctr["pingreqs"] > 0, ctr


@pytest.mark.parametrize("name", sorted(S.RECORD_WALKS))
def test_record_walk_shapes_have_rounds_in_which_every_live_row_holds_a_cold_member(name):
    quiet = S.rounds_without_hot_walks(OracleSim, name)
    print(f"{name}: rounds without a walk of the hot slots {quiet}")
    assert quiet and quiet[-1] == S.ROUNDS - 1


def test_three_round_case():
    ora = OracleSim(S.THREE_N)
    by_slot = []
    for r in range(3):
        rets = S.three_mutators(ora, r)
        assert all(x == 1 for x in rets), (r, rets)                 # every raw change applies
        by_slot.append(S.slot_bumps_expected(ora))
        if r == 1:                                                  # round B: the same senders hold a cold member
            assert all(set(ora.dis_entries(o)) == set(S.HOT + [S.COLD]) for o in S.SENDERS)
        if r == 2:                                                  # round C: their buffers are empty at issue
            assert all(not ora.dis_entries(o) for o in S.SENDERS)
        before = ora.counters()
        ora.step([])
        ctr = ora.counters()
        assert ctr["pings_ok"] - before["pings_ok"] == S.THREE_N    # every row pings and is answered
        assert ctr["timers_fired"] == 0
    assert set(S.SENDERS) <= set(by_slot[0])                        # round A: walks of the hot slots
    assert by_slot[1] and not set(S.SENDERS) & set(by_slot[1])      # round B: the senders' are not, other rows' are
    assert by_slot[2] and not set(S.SENDERS) & set(by_slot[2])
    # round C put a fresh entry (p = 0 at issue; sent at most by later messages) into a cleared row among those whose
    # cells the engine test reads back: the entry a bitmap of round A would wrongly bump
    fresh = [o for o in S.SENDERS[:3] if S.HOT[0] in ora.dis_entries(o)]
    assert fresh, [ora.dis_entries(o) for o in S.SENDERS[:3]]
    assert all(ora.dis_entries(o)[S.HOT[0]][0] == 0 for o in fresh)
