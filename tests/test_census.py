"""Member census and per-round member trace of the MI355X engine against the CPU oracle.

Every expected value comes from the oracle's rows() and live() alone: per member the bincount of the statuses the
counted observers hold it in (7 = unknown mapped to 5) and the smallest and largest incarnation over the rows that know
it. Equality is exact; no case is sampled.
"""
import numpy as np
import pytest

from oracle_ffi import OracleSim
import swimsim
from swimsim import metrics
from swimsim import workloads as W

pytestmark = pytest.mark.gpu

ORA_KW = ("t0_ms", "period_ms", "suspect_ms", "faulty_ms", "tombstone_ms", "ping_request_size", "max_rfs_jobs",
          "p_factor", "seed")


def make_pair(n, shards=0, **kw):
    init = kw.pop("init", "converged")
    eng = swimsim.ShardedCluster(n, shards, init=init, **kw) if shards else swimsim.Cluster(n, init=init, **kw)
    ora = OracleSim(n, init=init, **{k: v for k, v in kw.items() if k in ORA_KW})
    return eng, ora


def expected(ora, who="live", members=None):
    """(counts[n, 6], min_inc[n], max_inc[n]) of the oracle's state"""
    n = ora.n
    ost, oinc = ora.rows()
    mask = np.array([ora.live(o) for o in range(n)], bool) if who == "live" else np.ones(n, bool)
    cols = np.arange(n) if members is None else np.asarray(members, dtype=np.int64)
    st = np.where(ost == 7, 5, ost)[mask][:, cols]
    inc = oinc[mask][:, cols]
    counts = np.zeros((len(cols), 6), np.uint32)
    mn = np.full(len(cols), -1, np.int64)
    mx = np.full(len(cols), -1, np.int64)
    for j in range(len(cols)):
        counts[j] = np.bincount(st[:, j], minlength=6)
        known = inc[st[:, j] != 5, j]
        if len(known):
            mn[j], mx[j] = known.min(), known.max()
    return counts, mn, mx


def check(eng, ora, who, members=None, what=""):
    counts, mn, mx, ms = eng.census(members, who)
    n = ora.n if members is None else len(members)
    assert counts.shape == (n, 6) and mn.shape == (n,) and mx.shape == (n,)
    ec, emn, emx = expected(ora, who, members)
    bad = np.argwhere(counts != ec)
    assert not len(bad), f"{what} who={who}: counts of entry {bad[0][0]}: engine {counts[bad[0][0]]} oracle {ec[bad[0][0]]}"
    assert (mn == emn).all(), f"{what} who={who}: min incarnation differs at {np.nonzero(mn != emn)[0][:5]}"
    assert (mx == emx).all(), f"{what} who={who}: max incarnation differs at {np.nonzero(mx != emx)[0][:5]}"
    assert ms >= 0
    return counts, mn, mx


def step_both(eng, ora, events):
    evr = [e for e in events if e[0] == eng.round]
    eng.step(1, evr)
    ora.step(evr)


# ---- 1. the full census against the oracle, both `who` values ------------------------------------------------------

def scenario_config1():
    wl = W.config1()
    return make_pair(wl.n), wl.events, 32


def scenario_cascade():
    wl = W.config3(n=300, rounds=40, kill_round=3)
    return make_pair(wl.n), wl.events, wl.rounds


def scenario_eviction():
    # test_engine_parity.py::test_eviction_leave_reap_and_revive: leave, tombstone and evicted-as-unknown cells
    ev = [(0, W.EV_KILL, 3, 0), (2, W.EV_LEAVE, 7, 0), (4, W.EV_KILL, 9, 0), (30, W.EV_REAP, 1, 0),
          (40, W.EV_REVIVE, 3, 0), (41, W.EV_REINCARNATE, 11, 0)]
    return make_pair(24, faulty_ms=2000, tombstone_ms=1000), ev, 80


def scenario_self_only():
    # every node knows itself and learns members 0 and 1; a killed member is known to no live observer (-1 / -1)
    n = 65
    eng, ora = make_pair(n, init="self")
    for o in range(n):
        for m in (0, 1):
            if m != o:
                assert eng.make_change(o, m, swimsim.T0_MS, swimsim.ALIVE) == ora.make_change(o, m, swimsim.T0_MS, 0)
    return (eng, ora), [(0, W.EV_KILL, 10, 0), (0, W.EV_KILL, 64, 0)], 6


@pytest.mark.parametrize("scenario,first_checked", [(scenario_config1, 24), (scenario_cascade, 0), (scenario_eviction, 0),
                                                    (scenario_self_only, 0)])
def test_full_census_matches_oracle(scenario, first_checked):
    (eng, ora), events, rounds = scenario()
    seen = np.zeros(6, np.uint64)
    minus_one = False
    for r in range(rounds):
        step_both(eng, ora, events)
        if r < first_checked:
            continue
        for who in ("live", "all"):
            counts, mn, mx = check(eng, ora, who, what=f"round {r}")
            seen += counts.sum(axis=0).astype(np.uint64)
            minus_one |= bool((mn == -1).any() and (mx == -1).any())
    assert (eng.checksums() == ora.checksums()).all() and eng.digest() == ora.digest()
    if scenario is scenario_cascade:
        assert seen[1] and seen[2], "the cascade shows suspect and faulty cells"
    if scenario is scenario_eviction:
        assert seen[3] and seen[4] and seen[5], "the eviction scenario shows leave, tombstone and unknown cells"
    if scenario is scenario_self_only:
        assert seen[5] and minus_one, "the self-only start shows unknown cells and members no counted row knows"


@pytest.mark.parametrize("n", [1, 2, 3])
def test_full_census_tiny_clusters(n):
    eng, ora = make_pair(n)
    events = [(0, W.EV_KILL, n - 1, 0)] if n > 1 else []
    for r in range(12):
        step_both(eng, ora, events)
        for who in ("live", "all"):
            check(eng, ora, who, what=f"n={n} round {r}")


# ---- 2. tile edges -------------------------------------------------------------------------------------------------

EDGE_SIZES = [63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2112]


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_tile_edges(n):
    """One N just below, at and just above every bound of the kernels (csrc/swimsim_census.hip):
      63, 64, 65        the row padding NP (64 words) and the 64 lanes of k_census_cols' row groups
      255, 256, 257     CENSUS_WAVE_COLS = 256 columns per wave of k_census; CENSUS_COLS_CHUNK_ROWS = 256 rows per wave
                        of k_census_cols
      511, 512, 513     CENSUS_CHUNK_ROWS = 512 rows per slab of k_census (a full chunk is the largest value a packed
                        10-bit status counter carries); two full row chunks of k_census_cols
      1023, 1024, 1025  CENSUS_BLOCK_COLS = 1,024 columns per workgroup; two full row chunks of k_census
      2112              three workgroups of columns, five slabs, nine row chunks of k_census_cols
    A converged cluster holds every member alive in all N rows; then 20 members die and 8 rounds run in one call."""
    eng, ora = make_pair(n)
    counts, mn, mx, _ = eng.census(who="all")
    assert (counts[:, 0] == n).all() and (counts[:, 1:] == 0).all()
    assert (mn == swimsim.T0_MS).all() and (mx == swimsim.T0_MS).all()
    killed = [3 * i + 1 for i in range(20)]
    events = [(0, W.EV_KILL, m, 0) for m in killed]
    eng.step(8, events)
    ora.run(8, events)
    short = [0, n - 1, killed[0]]                                   # k_census_cols over the same row chunks
    for who in ("live", "all"):
        counts, _, _ = check(eng, ora, who, what=f"n={n}")
        check(eng, ora, who, short, what=f"n={n} list")
    assert (counts.sum(axis=1) == n).all()


# ---- 3. lists --------------------------------------------------------------------------------------------------------

def test_lists_either_side_of_the_switch_point():
    """A list of n members takes k_census_cols while n * CENSUS_LIST_WORDS (16) <= NP and k_census beyond. N = 300
    (NP = 320) switches after 20 members; N = 2,112 switches after 132, so its lists of 65 and 132 members loop
    k_census_cols' 64 lanes more than once."""
    wl = W.config3(n=300, rounds=12, kill_round=3)
    eng, ora = make_pair(wl.n)
    eng.step(12, wl.events)
    ora.run(12, wl.events)
    rng = np.random.default_rng(5)
    killed = [e[2] for e in wl.events]
    for who in ("live", "all"):
        full = eng.census(who=who)
        for k in (1, 20, 21, 64, 65):
            members = list(rng.choice(300, k, replace=False))
            members[0] = killed[0]
            counts, mn, mx = check(eng, ora, who, members, what=f"list of {k}")
            assert (counts == full[0][members]).all() and (mn == full[1][members]).all() and (mx == full[2][members]).all()
        for dup in ([killed[0], 5, killed[0]], [7] * 30):            # duplicates, on either path
            counts, _, _ = check(eng, ora, who, dup, what="duplicates")
            assert (counts[0] == counts[-1]).all()

    n = 2112
    eng, ora = make_pair(n)
    events = [(0, W.EV_KILL, m, 0) for m in range(100, 120)]
    eng.step(8, events)
    ora.run(8, events)
    for k in (64, 65, 132, 133):
        members = list(rng.choice(n, k, replace=False))
        members[-1] = 100
        check(eng, ora, "live", members, what=f"n={n} list of {k}")


# ---- 4. trace --------------------------------------------------------------------------------------------------------

def oracle_record(ora, tracked):
    counts, _, _ = expected(ora, "live", tracked)
    return ora.round - 1, sum(ora.live(o) for o in range(ora.n)), counts


def cascade_with_tracked(n=300, frac=0.02):
    wl = W.config3(n=n, rounds=40, kill_round=3, frac=frac)
    killed = [e[2] for e in wl.events]
    assert len(killed) >= 5
    alive = [m for m in range(1, n - 1) if m not in killed][:2]
    return wl, killed, killed[:5] + alive + [0, n - 1]


def test_trace_rounds_0_to_39_in_one_step():
    wl, killed, tracked = cascade_with_tracked()
    eng, ora = make_pair(wl.n)
    eng.trace_members(tracked, 64)
    eng.step(40, wl.events)
    want = []
    for _ in range(40):
        ora.step(wl.events_for(ora.round))
        want.append(oracle_record(ora, tracked))
    rounds, nlive, counts, dropped = eng.trace()
    assert dropped == 0 and list(rounds) == list(range(40))
    assert list(nlive) == [w[1] for w in want]
    assert counts.shape == (40, len(tracked), 6)
    for k in range(40):
        assert (counts[k] == want[k][2]).all(), f"round {k}: engine {counts[k]} oracle {want[k][2]}"
    # the trace disturbs nothing
    assert (eng.checksums() == ora.checksums()).all() and eng.digest() == ora.digest()
    assert eng.counters() == ora.counters()
    again = eng.trace()
    assert len(again[0]) == 0 and len(again[1]) == 0 and again[2].shape == (0, len(tracked), 6) and again[3] == 0
    got = metrics.detection_times(rounds, nlive, counts)
    ref = metrics.detection_times([w[0] for w in want], [w[1] for w in want], np.stack([w[2] for w in want]))
    assert got == ref
    for j in range(5):                                               # every killed member is suspected, then faulty
        assert got.first_suspect[j] is not None and got.first_suspect[j] >= 3
        assert got.first_faulty[j] is not None and got.first_faulty[j] > got.first_suspect[j]
    for j in range(5, len(tracked)):
        if tracked[j] not in killed:
            assert got.all_faulty[j] is None


def test_trace_capacity_drain_and_off():
    wl, killed, tracked = cascade_with_tracked()
    eng, ora = make_pair(wl.n)
    eng.trace_members(tracked, 8)
    eng.step(20, wl.events)
    want = []
    for _ in range(20):
        ora.step(wl.events_for(ora.round))
        want.append(oracle_record(ora, tracked))
    rounds, nlive, counts, dropped = eng.trace()
    assert list(rounds) == list(range(8)) and dropped == 12
    for k in range(8):
        assert nlive[k] == want[k][1] and (counts[k] == want[k][2]).all()
    eng.step(3, wl.events)                                           # it keeps recording after the drain
    for _ in range(3):
        ora.step(wl.events_for(ora.round))
        want.append(oracle_record(ora, tracked))
    rounds, nlive, counts, dropped = eng.trace()
    assert list(rounds) == [20, 21, 22] and dropped == 0
    for k in range(3):
        assert nlive[k] == want[20 + k][1] and (counts[k] == want[20 + k][2]).all()
    eng.trace_members(tracked[:2], 8)                                # a new set replaces the old one, records cleared
    eng.step(1, wl.events)
    ora.step(wl.events_for(ora.round))
    rounds, nlive, counts, dropped = eng.trace()
    assert list(rounds) == [23] and counts.shape == (1, 2, 6)
    assert (counts[0] == expected(ora, "live", tracked[:2])[0]).all()
    eng.trace_members([], 8)                                         # off
    eng.step(2, wl.events)
    ora.run(2, wl.events)
    rounds, nlive, counts, dropped = eng.trace()
    assert len(rounds) == 0 and dropped == 0
    assert (eng.checksums() == ora.checksums()).all() and eng.digest() == ora.digest()


def test_scratch_is_allocated_on_first_use_and_the_trace_is_freed():
    eng = swimsim.Cluster(300)
    eng.step(2)
    before = eng.memory()
    eng.trace_members([1, 2, 3], 1024)
    with_trace = eng.memory()
    assert with_trace["total"] >= before["total"] + 1024 * (2 + 6 * 3) * 4
    eng.trace_members([], 1)
    assert eng.memory() == before
    eng.census()
    eng.census([1, 2])
    after = eng.memory()
    assert after["total"] > before["total"]
    assert {k: v for k, v in after.items() if k != "total"} == {k: v for k, v in before.items() if k != "total"}
    eng.census()
    eng.census([2, 1])
    assert eng.memory() == after                                      # (the scratch is kept, not grown)


# ---- 5. shards -------------------------------------------------------------------------------------------------------

def test_sharded_census_and_trace():
    """ShardedCluster(100, 3) owns rows [0, 33), [33, 66), [66, 100): members 32 and 33 sit on either side of the first
    boundary; both are tracked, and observers 32 (killed with the cascade) and 33 (killed a round later) die."""
    n = 100
    wl = W.config3(n=n, rounds=40, kill_round=3, frac=0.05)
    events = wl.events + [(3, W.EV_KILL, 32, 0), (4, W.EV_KILL, 33, 0)]
    killed = sorted(set(e[2] for e in events))
    tracked = [32, 33, 31, 34, 65, 66] + [m for m in killed if m not in (32, 33)][:3]
    eng, ora = make_pair(n, shards=3)
    assert [c.lo for c in eng.shards] == [0, 33, 66]
    eng.trace_members(tracked, 64)
    eng.step(40, events)
    want = []
    for r in range(40):
        ora.step([e for e in events if e[0] == r])
        want.append(oracle_record(ora, tracked))
    rounds, nlive, counts, dropped = eng.trace()
    assert dropped == 0 and list(rounds) == list(range(40)) and list(nlive) == [w[1] for w in want]
    for k in range(40):
        assert (counts[k] == want[k][2]).all(), f"round {k}"
    assert (eng.checksums() == ora.checksums()).all() and eng.digest() == ora.digest()
    for who in ("live", "all"):
        check(eng, ora, who, what="sharded")
        check(eng, ora, who, [32, 33, killed[0]], what="sharded short list")        # 3 * 16 <= NP = 128: k_census_cols
        check(eng, ora, who, list(range(20, 40)), what="sharded long list")          # 20 * 16 > 128: k_census
    # a shard alone counts its own rows only
    ost, _ = ora.rows()
    c1 = eng.shards[1].census(who="all")[0]
    assert (c1.sum(axis=1) == 33).all()
    assert (c1[:, 0] == (ost[33:66] == 0).sum(axis=0)).all()


# ---- 6. errors -------------------------------------------------------------------------------------------------------

def test_errors_leave_the_next_call_correct():
    n = 40
    eng, ora = make_pair(n)
    events = [(0, W.EV_KILL, 4, 0)]
    eng.step(6, events)
    ora.run(6, events)
    L = swimsim.load_library()
    buf = np.zeros((n, 6), np.uint32)
    idx = np.arange(n, dtype=np.uint32)

    def ok():
        check(eng, ora, "live")
        check(eng, ora, "all", [4, 5])

    ok()
    assert L.swimsim_census(eng.h, None, n, 0, None, None, None, None) == -1                  # no counts
    ok()
    assert L.swimsim_census(eng.h, idx.ctypes.data, 0, 0, buf.ctypes.data, None, None, None) == -1   # n == 0
    with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
        eng.census([])
    ok()
    with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
        eng.census([1, n])                                                                    # an index >= N
    ok()
    assert L.swimsim_census(eng.h, None, n - 1, 0, buf.ctypes.data, None, None, None) == -1    # NULL members, n != N
    assert L.swimsim_census(eng.h, None, n + 1, 0, buf.ctypes.data, None, None, None) == -1
    ok()
    with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
        eng.census(who=2)                                                                     # an unknown who
    with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
        eng.census([1], who=-1)
    ok()
    # min / max pointers may be NULL, and so may ms
    assert L.swimsim_census(eng.h, None, n, 1, buf.ctypes.data, None, None, None) == 0
    assert (buf == expected(ora, "all")[0]).all()
    # the trace's errors leave no trace set and the engine intact
    for bad, cap in (([0] * 65, 8), ([n], 8), ([1, 2], 0), ([1, 2], 65537)):
        with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
            eng.trace_members(bad, cap)
    eng.step(1)
    ora.step([])
    assert len(eng.trace()[0]) == 0
    eng.trace_members([4, 5], 4)
    with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
        eng.trace_members([n + 3], 4)                                                         # the set in force stays
    eng.step(1)
    ora.step([])
    rounds, nlive, counts, dropped = eng.trace()
    assert list(rounds) == [7] and nlive[0] == n - 1 and (counts[0] == expected(ora, "live", [4, 5])[0]).all()
    ok()
    assert (eng.checksums() == ora.checksums()).all() and eng.digest() == ora.digest()
