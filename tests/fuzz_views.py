"""The read-only view calls on the states of the seeded random schedules (tests/fuzz_scenarios.py): census, route,
route_n, ring checksums and forwarding, each with its census. TEST INFRASTRUCTURE ONLY: no GPU work starts here; the
engine is whatever the caller hands in (tests/test_fuzz_views.py), and tests/test_fuzz_views_host.py runs the same
checkpoints on the CPU oracle alone.

Nothing is restated here. Every expected value comes from the helpers the hand-written scenarios already use:
test_census.check / expected, test_route.check_all / oracle_owners, test_route_n.check_all / oracle_prefs,
ring_checksum_scenarios.expected / expected_hist / check_hist and forward_cases.check_state / chase_grid / census. They
read `ora.n`, `ora.rows()` and `ora.live(o)` only, so RowsView (rows read back from the engine after a per-call record
proved them equal to the oracle's, with the schedule's liveness) can stand in for the oracle at 1,100 members.

The oracle has no partition read-back: Tracker follows the labels (set_partition mutators, EV_PARTITION events) and the
liveness (set_live, EV_KILL, EV_REVIVE) through the calls run so far, mutators before events as both sides run them.

check_views returns nothing; it notes what the state held in a reach dict (new_reach), which expected_views fills the
same way without an engine: the host test asserts on it what the schedules were measured to reach.
"""
import numpy as np

import forward_cases as FC
import fuzz_scenarios as F
import ring_checksum_scenarios as RS
import test_census as TC
import test_route as TR
import test_route_n as TRN

KEYS64 = TR.KEYS64
KEYS16 = KEYS64[:16]
SHORT_KEYS = 9                                    # the R = 1 pass: cnt * cnt * R <= N puts mode 0 on the direct path
REPLICAS = (3, 16)                                # the walk, and "every server" wherever a view holds at most 16
HOPS = (8, 1)
POLICIES = (FC.CHAIN, FC.ONE_HOP)
CASES = [(n, s) for n, s in F.CASES if n >= 5]
EVERY_CALL_UP_TO = 130                            # members; past it the first call, every fourth after it and the last
SAMPLED = 48


class Tracker:
    """partition labels and liveness of every member as the schedule has set them so far"""

    def __init__(self, n):
        self.part = np.zeros(n, np.int64)
        self.live = np.ones(n, bool)

    def apply(self, call):
        for m in call["muts"]:
            if m[0] == "set_partition":
                self.part[m[1]] = m[2]
            elif m[0] == "set_live":
                self.live[m[1]] = bool(m[2])
        for (_, k, a, b) in call["events"]:
            if k == F.EV_PARTITION:
                self.part[a] = b
            elif k in (F.EV_KILL, F.EV_REVIVE):
                self.live[a] = k == F.EV_REVIVE


class RowsView:
    """what the helpers read of an oracle, over rows read back from elsewhere: n, rows() and live(o)"""

    def __init__(self, rows, live):
        self.st, self.inc = rows
        self.n = len(live)
        self._live = np.asarray(live, bool).copy()

    def rows(self):
        return self.st, self.inc

    def live(self, o):
        return bool(self._live[o])


def checkpoint_calls(c):
    """the indices of the calls after which the views are checked"""
    k = len(c["calls"])
    if c["n"] <= EVERY_CALL_UP_TO:
        return set(range(k))
    return set(range(0, k, 4)) | {k - 1}


def traced_members(n):
    """min(n, 64) members for the trace: every ceil(n / 64)-th"""
    return list(range(0, n, -(-n // 64)))


def duplicate_lists(n):
    """member lists with duplicates: three entries (k_census_cols at every size) and every third member twice (k_census
    from 63 members on)"""
    return [[n - 1, 0, n - 1], list(range(0, n, 3)) * 2]


# ---- what a checked state held --------------------------------------------------------------------------------------

def new_reach():
    return {"checkpoints": 0, "rows": 0, "dead_rows": 0, "servers": {"empty": 0, "1-3": 0, "4-16": 0, ">16": 0},
            "distinct_views_max": 0, "cells": np.zeros(6, np.int64), "min_max_differ": 0, "incarnation_spread_max": 0,
            "ring_checksums_live_max": 0, "outcomes": np.zeros(6, np.int64), "listed_outcomes": np.zeros(6, np.int64),
            "split_keys": 0, "split_keys_max": 0, "disagreeing_keys": 0, "disagreeing_keys_max": 0,
            "replica_disagreeing_keys": 0}


def note(reach, live, counts, mn, mx, owners, prefs3, cs, srv, views, listed, fcensus):
    """add one checked state: the census of all rows, the owners, the replica sets at n = 3, the ring checksums and
    server counts, the listed forward of every entry and the forward census (chain, 8 hops; None where not run)"""
    reach["checkpoints"] += 1
    reach["rows"] += len(srv)
    reach["dead_rows"] += int((~live).sum())
    for name, lo, hi in (("empty", 0, 0), ("1-3", 1, 3), ("4-16", 4, 16), (">16", 17, 1 << 30)):
        reach["servers"][name] += int(((srv >= lo) & (srv <= hi)).sum())
    reach["distinct_views_max"] = max(reach["distinct_views_max"], views)
    reach["cells"] += counts.sum(axis=0).astype(np.int64)
    reach["min_max_differ"] += int((mn != mx).sum())
    reach["incarnation_spread_max"] = max(reach["incarnation_spread_max"], int((mx - mn).max()) // F.PERIOD_MS)
    reach["ring_checksums_live_max"] = max(reach["ring_checksums_live_max"], len(np.unique(cs[live])))
    dis = TR.disagreeing_keys(owners, live) if live.any() else 0
    reach["disagreeing_keys"] += dis
    reach["disagreeing_keys_max"] = max(reach["disagreeing_keys_max"], dis)
    if live.any():
        sets = np.sort(prefs3[live], axis=2)
        reach["replica_disagreeing_keys"] += int((sets != sets[0]).any(axis=(0, 2)).sum())
    if fcensus is not None:
        reach["outcomes"] += fcensus[1].sum(axis=0).astype(np.int64)
        reach["listed_outcomes"] += np.bincount(listed[0].ravel(), minlength=6)
        split = FC.split_keys(fcensus)
        reach["split_keys"] += split
        reach["split_keys_max"] = max(reach["split_keys_max"], split)


def expected_views(ora, part, keys, *, R, reach):
    """the expectations of one checkpoint on the oracle alone, noted in reach: what check_views compares an engine with"""
    live = RS.live_mask(ora, "live")
    counts, mn, mx = TC.expected(ora, "all")
    owners = TR.oracle_owners(ora, keys, R)
    prefs3, _ = TRN.oracle_prefs(ora, keys, 3, R)
    cs, srv, views = RS.expected(ora)
    listed = FC.chase_grid(owners, live, part, np.arange(ora.n), HOPS[0])
    note(reach, live, counts, mn, mx, owners, prefs3, cs, srv, views, listed, FC.census(owners, live, part, HOPS[0]))


# ---- an engine against the expectations -----------------------------------------------------------------------------

def check_census(eng, ora, what):
    """census of all members and of lists with duplicates, who = live and all; returns the who = all result"""
    for who in ("live", "all"):
        res = TC.check(eng, ora, who, what=what)
        for members in duplicate_lists(ora.n):
            TC.check(eng, ora, who, members, what=f"{what} list of {len(members)}")
    return res


def check_ring(eng, ora, what):
    """ring_checksums of the live rows and of all rows, and ring_census with both who values, in every mode; returns the
    oracle's (checksums, servers, distinct views)"""
    cs, srv, views = RS.expected(ora)
    for mode in RS.MODES:
        for who in ("live", "all"):
            mask = RS.live_mask(ora, who)
            obs = None if who == "all" else np.nonzero(mask)[0]
            if obs is None or len(obs):                             # (a call without observers is refused)
                got, gsrv, hashed, _ = eng.ring_checksums(obs, mode)
                bad = np.nonzero(got != cs[mask])[0]
                assert got.shape == cs[mask].shape and not len(bad), (
                    f"{what} mode {mode} who={who}: row {np.nonzero(mask)[0][bad[0]]}: engine {got[bad[0]]} oracle "
                    f"{cs[mask][bad[0]]} ({len(bad)} differ)")
                assert (gsrv == srv[mask]).all(), f"{what} mode {mode} who={who}: server counts differ"
                assert 1 <= hashed <= len(got)
            RS.check_hist(eng.ring_census(who, mode), RS.expected_hist(cs, srv, mask), f"{what} mode {mode} who={who}")
    return cs, srv, views


def check_views(eng, ora, part, keys, *, R, what, forward=True, reach=None):
    """every view call of eng against the restatements over ora's state (n, rows(), live(o)) and the partition labels
    part, exactly, for every row and every key; forward=False leaves the forward calls out (a sharded cluster)"""
    live = RS.live_mask(ora, "live")
    counts, mn, mx = check_census(eng, ora, what)
    owners = TR.check_all(eng, ora, keys, R=R, what=what)
    TR.check_all(eng, ora, keys[:SHORT_KEYS], R=1, what=f"{what} R=1")
    prefs = TRN.check_all(eng, ora, keys, ns=REPLICAS, R=R, what=what)
    cs, srv, views = check_ring(eng, ora, what)
    listed = fcensus = None
    if forward:
        for hops in HOPS:
            for policy in POLICIES:
                res = FC.check_state(eng, owners, live, part, keys, hops, policy, R, what=f"{what} hops {hops} policy {policy}")
                if (hops, policy) == (HOPS[0], FC.CHAIN):
                    listed, fcensus = res
    if reach is not None:
        note(reach, live, counts, mn, mx, owners, prefs[3], cs, srv, views, listed, fcensus)


# ---- at 1,100 members: all rows at R = 2, sampled observers at R = 100 -----------------------------------------------

def sampled_observers(c, tracker):
    """SAMPLED observers of a mass case: 0, n - 1, the first member the schedule kills and the first it cuts off, a row
    that is dead now and one outside partition 0 now (where there is one), the rest evenly spread"""
    n = c["n"]
    ev = [e for call in c["calls"] for e in call["events"]]
    pick = [0, n - 1, next(a for (r, k, a, b) in ev if (r, k) == (F.MASS_KILL_ROUND, F.EV_KILL)),
            next(a for (r, k, a, b) in ev if (r, k, b) == (F.MASS_CUT_ROUND, F.EV_PARTITION, 1))]
    pick += [int(x[0]) for x in (np.nonzero(~tracker.live)[0], np.nonzero(tracker.part)[0]) if len(x)]
    out = list(dict.fromkeys(pick))
    for o in range(7, n, n // SAMPLED):
        if len(out) < SAMPLED and o not in out:
            out.append(o)
    return out


def owners_closure(view, keys, R, entries, hops):
    """(owners[n, K], known[n]): the owners of every row a chain of at most `hops` forwards from the entries can visit;
    the other rows hold -2, which no such chain reads"""
    owners = np.full((view.n, len(keys)), -2, np.int32)
    known = np.zeros(view.n, bool)
    front = np.unique(np.asarray(entries, np.int64))
    for _ in range(hops + 1):
        front = front[~known[front]]
        if not len(front):
            break
        owners[front] = TR.oracle_owners(view, keys, R, rows=front)
        known[front] = True
        dest = np.unique(owners[front])
        front = dest[dest >= 0].astype(np.int64)
    return owners, known


def check_views_at_size(eng, view, part, sample, *, what, forward=True, keys=KEYS16, R_all=2, R_sample=100):
    """The view calls on one state of a mass schedule. view = RowsView(eng.rows(), the schedule's liveness).
    All rows: the census, the ring checksums and their census, and route / route_census, route_n / replica_census and
    forward / forward_census at R_all. The sampled observers: route, route_n and the listed forward at R_sample."""
    live = RS.live_mask(view, "live")
    check_census(eng, view, what)
    check_ring(eng, view, what)
    owners = TR.check_all(eng, view, keys, R=R_all, what=f"{what} R={R_all}")
    TRN.check_all(eng, view, keys, ns=(3,), R=R_all, what=f"{what} R={R_all}")
    if forward:
        FC.check_state(eng, owners, live, part, keys, HOPS[0], FC.CHAIN, R_all, what=f"{what} R={R_all}")
    what = f"{what} R={R_sample} sampled"
    if forward:
        owners, known = owners_closure(view, keys, R_sample, sample, HOPS[0])
        want = FC.chase_grid(owners, live, part, sample, HOPS[0])
        assert known[want[3]].all() and (want[4] >= -1).all()        # every row the chains read is one of the closure
        for mode in FC.MODES:
            FC.check_listed(eng.forward(keys, sample, None, HOPS[0], "chain", R_sample, mode), want, f"{what} mode {mode}")
        want = owners[sample]
    else:
        want = TR.oracle_owners(view, keys, R_sample, rows=sample)
    for mode in TR.MODES:
        got = eng.route(keys, sample, R_sample, mode)
        bad = np.argwhere(got != want)
        assert got.shape == want.shape and not len(bad), (
            f"{what} mode {mode}: observer {sample[bad[0][0]]} key {keys[bad[0][1]]!r}: engine {got[tuple(bad[0])]} "
            f"expected {want[tuple(bad[0])]} ({len(bad)} differ)")
    n = REPLICAS[-1]                                                 # (every view here holds more servers: the walk)
    want, srv = TRN.oracle_prefs(view, keys, n, R_sample, rows=sample)
    for mode in TR.MODES:
        got, gsrv = eng.route_n(keys, sample, n, R_sample, mode)
        TRN.check_lists(got, gsrv, want, srv, keys, f"{what} n {n} mode {mode}")
