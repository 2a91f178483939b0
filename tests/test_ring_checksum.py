"""Ring checksums through every node's own ring view (swimsim_ring_checksums, swimsim_ring_census) against the CPU
oracle.

Every expected value comes from the oracle alone: OracleSim.rows() and live() give the views, and
oracle_ffi.fingerprint32 hashes the addresses a row holds alive or suspect, in ascending member order, joined by ';'
(once per distinct presence set: ring_checksum_scenarios.expected_rows). Equality is exact: every row, nothing sampled.
Modes 0 (equal views share a chain), 1 (one chain per row) and 2 (grouping keys of 3 bits: only the exact comparison
parts unequal views) must agree.
"""
from contextlib import closing

import numpy as np
import pytest

import address_scenarios as S
from oracle_ffi import OracleSim
import ring_checksum_scenarios as RS
import swimsim
from swimsim import metrics
from swimsim import workloads as W
from test_census import make_pair, scenario_config1, scenario_eviction, scenario_self_only, step_both

pytestmark = pytest.mark.gpu

MODES = RS.MODES
CHUNK = swimsim.RING_CHECKSUM_CHUNK


def check_rows(eng, want, observers, what, modes=MODES):
    """ring_checksums of the listed observers (None: all) in every mode against want = (checksums, servers) of those rows"""
    out = {}
    for mode in modes:
        cs, srv, hashed, ms = eng.ring_checksums(observers, mode)
        assert cs.dtype == np.uint32 and cs.shape == want[0].shape and srv.shape == want[1].shape
        bad = np.nonzero(cs != want[0])[0]
        assert not len(bad), (f"{what} mode {mode}: row {bad[0]} of {want[1][bad[0]]} servers: engine {cs[bad[0]]} oracle "
                              f"{want[0][bad[0]]} ({len(bad)} of {len(cs)} differ)")
        assert (srv == want[1]).all(), f"{what} mode {mode}: server counts differ at {np.nonzero(srv != want[1])[0][:5]}"
        assert 1 <= hashed <= len(cs) and ms >= 0
        out[mode] = hashed
    return out


def check_all(eng, ora, addresses=None, what="", modes=MODES, whos=("live", "all")):
    """every row and the census with both who values, in every mode; returns the oracle's (checksums, servers, views)"""
    cs, srv, views = RS.expected(ora, addresses)
    hashed = check_rows(eng, (cs, srv), None, what, modes)
    if 0 in hashed:
        assert hashed[0] == views, f"{what}: {hashed[0]} chains for {views} distinct views (a 64-bit key collision: p < 1e-15)"
    if 1 in hashed:
        assert hashed[1] == ora.n
    for mode in modes:
        for who in whos:
            RS.check_hist(eng.ring_census(who, mode), RS.expected_hist(cs, srv, RS.live_mask(ora, who)),
                          f"{what} mode {mode} who={who}")
    return cs, srv, views


# ---- 1. scenarios ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scenario,first_checked", [(scenario_config1, 24), (scenario_eviction, 0), (scenario_self_only, 0)])
def test_scenarios_match_oracle(scenario, first_checked):
    (eng, ora), events, rounds = scenario()
    try:
        counts = set()
        for r in range(rounds):
            step_both(eng, ora, events)
            if r < first_checked:
                continue
            _, srv, _ = check_all(eng, ora, what=f"round {r}")
            counts |= set(int(x) for x in srv)
        assert (eng.checksums() == ora.checksums()).all() and eng.digest() == ora.digest()
        if scenario is scenario_eviction:
            assert len(counts) >= 3, "the eviction scenario shows views of several sizes"
        if scenario is scenario_self_only:
            assert min(counts) <= 3, "the self-only start shows views of one to three servers"
    finally:
        eng.close()


# ---- 2. the cascade, 6. grouping, 11. façade -------------------------------------------------------------------------

def test_cascade_rounds_distinct_checksums_grouping_and_facade():
    wl = RS.cascade_workload()
    eng, ora = make_pair(wl.n)
    try:
        for r in range(wl.rounds):
            step_both(eng, ora, wl.events)
            if r not in RS.CASCADE_CHECKED:
                continue
            cs, srv, views = check_all(eng, ora, what=f"cascade round {r}")
            assert 297 <= srv.min() and srv.max() <= 300
            live = RS.live_mask(ora, "live")
            if r in RS.CASCADE_DISTINCT:
                got = tuple(eng.ring_census(who)[1].size for who in ("live", "all"))
                assert got == RS.CASCADE_DISTINCT[r], f"round {r}: distinct ring checksums {got}"
            ag = metrics.ring_agreement(*eng.ring_census("live")[:3])
            if r in (2, 39):
                assert ag.all_agree and ag.share == 1.0 and ag.checksum == int(cs[live][0])
            if r == 30:
                assert not ag.all_agree and ag.distinct == 8 and 0 < ag.share < 1
                # grouping over the live rows alone: one chain per distinct view in mode 0, one per row in mode 1
                obs = np.nonzero(live)[0]
                nviews = RS.distinct_views(ora.rows()[0], live)
                assert nviews == 8
                hashed = check_rows(eng, (cs[obs], srv[obs]), obs, "cascade round 30, live rows")
                assert hashed[0] == nviews, f"{hashed[0]} chains for {nviews} views (a 64-bit key collision: p < 1e-15)"
                assert hashed[1] == len(obs)
                assert hashed[0] <= hashed[2] <= hashed[1]
                for o in (0, int(obs[-1]), int(np.nonzero(~live)[0][0])):
                    assert swimsim.Node(eng, o).Checksum() == int(cs[o])
    finally:
        eng.close()


# ---- 3. every address width --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", S.WIDTHS)
def test_every_address_width(w):
    n = 96
    kw, start, ev = S.scenario(n, "A")
    addrs = S.addresses(n, w)
    with closing(swimsim.Cluster(n, addresses=addrs, **kw)) as eng:
        ora = OracleSim(n, addresses=addrs, **kw)
        residues = set()
        for r in range(20):
            step_both(eng, ora, ev)
            if r < 8:
                continue
            _, srv, _ = check_all(eng, ora, addrs, what=f"w={w} round {r}")
            assert 83 <= srv.min() and srv.max() <= 96
            residues |= set(int(c) * (w + 1) % 20 for c in srv)       # (len + 1) mod 20
        assert len(residues) >= 2 or w == 19


# ---- 4. length edges -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", S.WIDTHS)
def test_length_edges(w):
    """row o holds exactly o servers: cnt = 0 (the empty string), cnt = 1 (one address: the 13-to-24 path) and every
    string length 2 w + 1 .. 47 (w + 1) - 1 in steps of w + 1, so every block-boundary residue the width allows and the
    last 20 bytes at every offset in the last two records; once as a prefix of the members, once scattered"""
    n = 48
    addrs = S.addresses(n, w, w & 1)
    inc = np.full(n, swimsim.T0_MS, np.int64)
    for scattered in (False, True):
        with closing(swimsim.Cluster(n, addresses=addrs)) as eng:
            ora = OracleSim(n, addresses=addrs)
            for o in range(n):
                st = np.full(n, swimsim.UNKNOWN, np.uint8)
                members = [(7 * i + o) % n for i in range(o)] if scattered else list(range(o))
                for i, m in enumerate(members):
                    st[m] = swimsim.ALIVE if i % 3 else swimsim.SUSPECT
                eng.set_row(o, st, inc)
                ora.set_row(o, st, inc)
            cs, srv, views = check_all(eng, ora, addrs, what=f"w={w} scattered={scattered}", whos=("all",))
            assert list(srv) == list(range(n)) and views == n
            assert cs[0] == RS.EMPTY


# ---- 5. chunk boundaries ---------------------------------------------------------------------------------------------

def test_chunk_boundaries():
    n = 2 * CHUNK + 77
    edges = [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1]
    rows = {}
    rows[3] = np.ones(n, bool)                                         # all present
    rows[n - 1] = np.ones(n, bool)
    rows[n - 1][edges] = False                                         # absent just below, at and just above each boundary
    rows[CHUNK] = np.zeros(n, bool)
    rows[CHUNK][2 * CHUNK:] = True                                     # present only inside the last chunk
    rows[CHUNK - 1] = np.zeros(n, bool)
    rows[CHUNK - 1][[0, n - 1]] = True                                 # only member 0 and member n - 1
    rows[2 * CHUNK] = np.zeros(n, bool)
    rows[2 * CHUNK][CHUNK] = True                                      # a single member
    rows[7] = np.zeros(n, bool)                                        # none
    rows[8] = np.zeros(n, bool)
    rows[8][edges] = True                                              # present only at the boundaries
    rows[2 * CHUNK + 1] = np.ones(n, bool)
    rows[2 * CHUNK + 1][CHUNK:2 * CHUNK] = False                       # an empty middle chunk
    assert len(rows) == 8
    inc = np.full(n, swimsim.T0_MS, np.int64)
    with closing(swimsim.Cluster(n)) as eng:
        ora = OracleSim(n)
        for o, present in rows.items():
            st = np.where(present, swimsim.ALIVE, swimsim.FAULTY).astype(np.uint8)
            eng.set_row(o, st, inc)
            ora.set_row(o, st, inc)
        obs = sorted(rows) + [5, n - 2]                                # two untouched rows
        status = np.stack([ora.row(o)[0] for o in obs])
        cs, srv, views = RS.expected_rows(status)
        assert views == 8 and cs[obs.index(7)] == RS.EMPTY and sorted(srv)[:3] == [0, 1, 2]
        hashed = check_rows(eng, (cs, srv), obs, "chunk boundaries")
        assert hashed[0] == views and hashed[1] == len(obs)
        assert cs[obs.index(5)] == cs[obs.index(3)] == cs[obs.index(n - 2)]


# ---- 7. tiny clusters ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65])
def test_tiny_clusters(n):
    eng, ora = make_pair(n)
    try:
        events = [(0, W.EV_LEAVE, 0, 0)] if n > 1 else []
        check_all(eng, ora, what=f"n={n} at the start")
        for r in range(8):
            step_both(eng, ora, events)
            check_all(eng, ora, what=f"n={n} round {r}")
    finally:
        eng.close()


# ---- 8. read-only ------------------------------------------------------------------------------------------------------

def test_calls_are_read_only_and_scratch_comes_at_first_use():
    wl = W.config3(n=300, rounds=30, kill_round=3)
    eng, ora = make_pair(wl.n)
    other = swimsim.Cluster(wl.n)
    try:
        for r in range(12):
            step_both(eng, ora, wl.events)
        other.step(12, wl.events)
        before = (eng.digest(), eng.checksums().copy(), eng.counters())
        mem0, mem_other = eng.memory()["total"], other.memory()["total"]
        assert mem0 == mem_other
        check_all(eng, ora, what="round 11")
        mem1 = eng.memory()["total"]
        assert mem0 < mem1 <= mem0 + (1 << 20), "the scratch is allocated at the first call"
        check_all(eng, ora, what="round 11 again")
        assert eng.memory()["total"] == mem1 and other.memory()["total"] == mem_other
        after = (eng.digest(), eng.checksums(), eng.counters())
        assert before[0] == after[0] and (before[1] == after[1]).all() and before[2] == after[2]
        for r in range(10):                                           # and the rounds go on in parity
            step_both(eng, ora, wl.events)
        assert (eng.checksums() == ora.checksums()).all() and eng.digest() == ora.digest()
        check_all(eng, ora, what="round 21", modes=(0,))
    finally:
        eng.close()
        other.close()


# ---- 9. shards ---------------------------------------------------------------------------------------------------------

def test_shards_answer_their_rows_and_histograms_merge():
    wl = RS.cascade_workload()
    eng, ora = make_pair(wl.n, shards=3)
    try:
        for r in range(34):
            step_both(eng, ora, wl.events)
            if r not in (30, 33):
                continue
            cs, srv, _ = RS.expected(ora)
            for mode in MODES:
                got, gsrv, hashed, ms = eng.ring_checksums(None, mode)
                assert (got == cs).all() and (gsrv == srv).all(), f"round {r} mode {mode}"
                for who in ("live", "all"):
                    RS.check_hist(eng.ring_census(who, mode), RS.expected_hist(cs, srv, RS.live_mask(ora, who)),
                                  f"3 shards round {r} mode {mode} who={who}")
            obs = [299, 0, 150, 150, 101]                              # any order, over all shards, a duplicate
            got, gsrv, _, _ = eng.ring_checksums(obs)
            assert (got == cs[obs]).all() and (gsrv == srv[obs]).all()
            c = eng.shards[1]                                          # a shard answers for its own rows only
            RS.check_hist(c.ring_census("all"), RS.expected_hist(cs[c.lo:c.lo + c.nl], srv[c.lo:c.lo + c.nl],
                                                                 np.ones(c.nl, bool), c.lo), f"shard 1 round {r}")
            with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
                c.ring_checksums([0])
    finally:
        eng.close()


# ---- 10. errors ------------------------------------------------------------------------------------------------------

def test_errors_are_refused_and_the_handle_stays_usable():
    import ctypes as C
    n = 70
    eng, ora = make_pair(n)
    try:
        L = swimsim.load_library()
        obs = np.arange(4, dtype=np.uint32)
        cs = np.full(4, 77, np.uint32)
        hist = [np.full(4, 9, np.uint32) for _ in range(4)]
        counted, nh = C.c_uint32(5), C.c_size_t(6)

        def rows(observers, nobs, mode, out=cs):
            return L.swimsim_ring_checksums(eng.h, None if observers is None else observers.ctypes.data, nobs, mode,
                                            None if out is None else out.ctypes.data, None, None, None)

        def census(who, mode, counted_p=C.byref(counted), nh_p=C.byref(nh), bufs=hist, cap=4):
            return L.swimsim_ring_census(eng.h, who, mode, counted_p, *(None if b is None else b.ctypes.data for b in bufs),
                                         cap, nh_p, None, None)

        assert rows(obs, 4, 0, None) == -1                             # no output
        assert rows(obs, 0, 0) == -1                                   # nobs = 0
        assert rows(None, n - 1, 0) == -1                              # every row means nobs = the owned rows
        assert rows(np.array([0, n], np.uint32), 2, 0) == -1           # out of range
        assert rows(obs, 4, 3) == -1 and rows(obs, 4, -1) == -1        # unknown mode
        assert b"mode" in L.swimsim_last_error(eng.h)
        assert (cs == 77).all()
        assert census(2, 0) == -1 and census(-1, 0) == -1              # unknown who
        assert census(0, 3) == -1                                      # unknown mode
        assert census(0, 0, counted_p=None) == -1 and census(0, 0, nh_p=None) == -1
        assert census(0, 0, bufs=[hist[0], None, hist[2], hist[3]]) == -1
        assert counted.value == 5 and nh.value == 6 and all((b == 9).all() for b in hist)
        with pytest.raises(ValueError):
            eng.ring_census("some")
        with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
            eng.ring_checksums([])
        check_all(eng, ora, what="after the refused calls")
        assert census(0, 0, bufs=[None] * 4, cap=0) == 0               # cap = 0: the count alone
        assert counted.value == n and nh.value == 1
        # no counted rows
        for m in range(n):
            eng.set_live(m, False)
        got = eng.ring_census("live")
        assert got[0] == 0 and all(len(got[i]) == 0 for i in range(1, 5)) and got[5] == 0
        assert eng.ring_census("all")[0] == n
    finally:
        eng.close()


# ---- 12. one run at size -----------------------------------------------------------------------------------------------

def test_one_run_at_size():
    wl = W.config2(n=4096, rounds=6)
    eng, ora = make_pair(wl.n)
    try:
        eng.step(wl.rounds, wl.events)
        ora.run(wl.rounds, wl.events)
        cs, srv, views = RS.expected(ora)
        got, gsrv, hashed, ms = eng.ring_checksums(None, 0)
        bad = np.nonzero(got != cs)[0]
        assert not len(bad), f"row {bad[:5]}: engine {got[bad[:5]]} oracle {cs[bad[:5]]} ({len(bad)} differ)"
        assert (gsrv == srv).all()
        assert hashed == views, f"{hashed} chains for {views} distinct views (a 64-bit key collision: p < 1e-12)"
        RS.check_hist(eng.ring_census("all", 0), RS.expected_hist(cs, srv, np.ones(wl.n, bool)), "n=4096 who=all")
    finally:
        eng.close()
