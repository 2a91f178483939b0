"""Key routing through every node's own ring view (swimsim_route, swimsim_route_census) against the CPU oracle.

Every expected value comes from the oracle alone: OracleSim.rows() and live() give the views, one fresh
OracleRing(R).add_remove_servers(...) is built per observer row from the members the row holds alive or suspect, in
ascending member order (once per distinct set of such members: equal sets build equal rings), and OracleRing.lookup
answers every key. Equality is exact: every row, every key, nothing
sampled. The oracle's owners of one state are computed once and compared with the engine in modes 0 (automatic), 1 (ring
walk) and 2 (direct path wherever the row fits the list), which must agree.
"""
import ctypes as C
import os

import numpy as np
import pytest

import address_scenarios as S
from oracle_ffi import OracleRing, OracleSim, fingerprint32
import swimsim
from swimsim import metrics
from swimsim import workloads as W
from test_census import make_pair, scenario_eviction, scenario_self_only, step_both

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2)
KEYS64 = [f"key-{i}" for i in range(64)]


def oracle_owners(ora, keys, R=100, addresses=None, rows=None):
    """owners[rows, K] (int32, -1: empty ring) of the oracle's state, every observer row by default"""
    n = ora.n
    addr = list(addresses) if addresses is not None else [swimsim.address_of(m) for m in range(n)]
    index = {a: m for m, a in enumerate(addr)}
    ost, _ = ora.rows()
    rows = list(range(n)) if rows is None else list(rows)
    out = np.empty((len(rows), len(keys)), np.int32)
    views = answers_of("owners", R, addr if addresses is not None else n, keys)
    for j, o in enumerate(rows):
        present = ost[o] <= 1
        view = present.tobytes()
        if view not in views:
            ring = OracleRing(R)
            ring.add_remove_servers([addr[m] for m in np.nonzero(present)[0]], [])
            views[view] = [index[a] if ok else -1 for a, ok in (ring.lookup(key) for key in keys)]
        out[j] = views[view]
    return out


# The oracle ring's answers per view, kept for the session: rows that hold the same members alive or suspect have the same
# ring, and a ring's answers are a function of (what is asked, R, the addresses, the keys, the view) alone. The states of
# a schedule repeat most views from call to call, and its sharded and variant runs repeat all of them.
_ANSWERS = {}
ANSWERS_CAP = 60_000                            # views over all tables; past it the tables start again


def answers_of(what, R, addresses, keys):
    """the table {view bytes: answers} of one question; addresses = the address list, or n for the synthetic ones"""
    if sum(len(t) for t in _ANSWERS.values()) > ANSWERS_CAP:
        _ANSWERS.clear()
    ident = (what, R, addresses if isinstance(addresses, int) else tuple(addresses), tuple(keys))
    return _ANSWERS.setdefault(ident, {})


def cascade_keys(wl):
    """64 keys for the cascade workload: key-0 .. key-39 and, for each killed member, the first 8 keys "key-i" the ring
    of all members gives to it (so that the checked keys include some whose owner dies)"""
    killed = sorted(e[2] for e in wl.events)
    ring = OracleRing(100)
    addr = [swimsim.address_of(m) for m in range(wl.n)]
    ring.add_remove_servers(addr, [])
    keys, found, i = [f"key-{i}" for i in range(40)], {addr[m]: 0 for m in killed}, 40
    while len(keys) < 40 + 8 * len(killed):
        a, _ = ring.lookup(f"key-{i}")
        if found.get(a, 8) < 8:
            found[a] += 1
            keys.append(f"key-{i}")
        i += 1
    return keys


def expected_hist(owners, mask):
    """(counted, hist_off, hist_owner, hist_count) of the rows in mask"""
    counted = int(mask.sum())
    off, own, cnt = [0], [], []
    for k in range(owners.shape[1]):
        u, c = np.unique(owners[mask, k], return_counts=True)         # ascending: -1 first
        own += list(u)
        cnt += list(c)
        off.append(len(own))
    return counted, np.array(off, np.uint64), np.array(own, np.int32), np.array(cnt, np.uint32)


def live_mask(ora, who):
    return np.array([ora.live(o) for o in range(ora.n)], bool) if who == "live" else np.ones(ora.n, bool)


def check_hist(got, want, what, per_key=None):
    """exact, every key; the counts of a key sum to per_key (route_census: one owner per counted row)"""
    counted, off, own, cnt = got[:4]
    per_key = want[0] if per_key is None else per_key
    assert counted == want[0], f"{what}: counted {counted}, oracle {want[0]}"
    assert (off == want[1]).all(), f"{what}: hist_off differs at key {np.nonzero(off != want[1])[0][:3]}"
    assert len(own) == len(want[2]) and (own == want[2]).all() and (cnt == want[3]).all(), f"{what}: histogram entries differ"
    for k in range(len(off) - 1):
        assert int(cnt[int(off[k]):int(off[k + 1])].sum()) == per_key
    assert got[4] >= 0


def check_all(eng, ora, keys, R=100, addresses=None, what="", modes=MODES):
    """route of every observer and route_census with live and all, in every mode; returns the oracle's owners"""
    want = oracle_owners(ora, keys, R, addresses)
    for mode in modes:
        got = eng.route(keys, list(range(ora.n)), R, mode)
        assert got.shape == want.shape and got.dtype == np.int32
        bad = np.argwhere(got != want)
        assert not len(bad), (f"{what} mode {mode}: observer {bad[0][0]} key {keys[bad[0][1]]!r}: engine "
                              f"{got[bad[0][0], bad[0][1]]} oracle {want[bad[0][0], bad[0][1]]} ({len(bad)} differ)")
        for who in ("live", "all"):
            check_hist(eng.route_census(keys, who, R, mode), expected_hist(want, live_mask(ora, who)),
                       f"{what} mode {mode} who={who}")
    return want


def disagreeing_keys(owners, mask):
    return int(sum(len(np.unique(owners[mask, k])) > 1 for k in range(owners.shape[1])))


# ---- 1. scenarios ---------------------------------------------------------------------------------------------------

CASCADE_ROUNDS = (2, 5) + tuple(range(27, 35)) + (39,)


def test_cascade():
    """W.config3(n=300, kill_round=3): N is no multiple of 64. The three killed members turn suspect (still servers)
    and then, node by node, faulty in rounds 28 to 32 (suspect timeout of 25 rounds): there the live nodes disagree on
    the keys the killed members owned. From round 33 on the live nodes agree again and only the killed nodes' own rows,
    which who = "all" counts, still answer the old owners."""
    wl = W.config3(n=300, rounds=40, kill_round=3)
    assert len(wl.events) == 3
    keys = cascade_keys(wl)
    assert len(keys) == 64
    eng, ora = make_pair(wl.n)
    try:
        disagree = {}
        for r in range(40):
            step_both(eng, ora, wl.events)
            if r in CASCADE_ROUNDS:
                want = check_all(eng, ora, keys, what=f"round {r}")
                disagree[r] = (disagreeing_keys(want, live_mask(ora, "live")), disagreeing_keys(want, live_mask(ora, "all")))
        assert disagree[2] == (0, 0) and disagree[30][0] == 24 and disagree[39] == (0, 24), disagree
        assert (eng.checksums() == ora.checksums()).all() and eng.digest() == ora.digest()
    finally:
        eng.close()


def test_eviction():
    """leave, tombstone and unknown (evicted) cells are not servers"""
    (eng, ora), events, rounds = scenario_eviction()
    try:
        seen = set()
        for r in range(rounds):
            step_both(eng, ora, events)
            if r % 4 == 0 or r in (2, 3, 5, 31, 41, 42):
                check_all(eng, ora, KEYS64, what=f"round {r}")
                seen |= set(np.unique(ora.rows()[0]))
        assert {3, 4, 7} <= seen, "the checked rounds show leave, tombstone and unknown cells"
    finally:
        eng.close()


def test_self_only_start():
    """n = 65, every node knows itself and members 0 and 1: rings of 1 to 3 members, which mode 0 routes on the direct
    path (cnt * cnt * R <= N holds for no such ring at N = 65 and R = 100, so the same rows are also routed with R = 1,
    where it holds for cnt <= 8). Members 10 and 64 are killed: who = "all" counts their rows, who = "live" does not."""
    (eng, ora), events, rounds = scenario_self_only()
    try:
        for r in range(rounds):
            step_both(eng, ora, events)
            check_all(eng, ora, KEYS64, what=f"round {r}")
            check_all(eng, ora, KEYS64[:9], R=1, what=f"round {r} R=1")
        assert not ora.live(10) and not ora.live(64)
        assert eng.route_census(KEYS64, "all")[0] == 65 and eng.route_census(KEYS64, "live")[0] == 63
    finally:
        eng.close()


def test_single_node():
    eng, ora = make_pair(1)
    try:
        for r in range(3):
            step_both(eng, ora, [])
            want = check_all(eng, ora, KEYS64[:5], what=f"n=1 round {r}")
            assert (want == 0).all()
    finally:
        eng.close()


def test_one_replica_point_three_nodes():
    """R = 1 with N = 3: three points, most keys wrap to the first"""
    eng, ora = make_pair(3)
    try:
        events = [(1, W.EV_KILL, 2, 0)]
        for r in range(4):
            step_both(eng, ora, events)
            check_all(eng, ora, KEYS64, R=1, what=f"R=1 round {r}")
        top = max(h for h, _ in _points(1, 3))
        assert sum(fingerprint32(k.encode()) > top for k in KEYS64), "some key hashes above every point"
    finally:
        eng.close()


def _points(R, n):
    ring = OracleRing(R)
    ring.add_remove_servers([swimsim.address_of(m) for m in range(n)], [])
    return ring.points()


def test_thousand_replica_points():
    """R = 1000: three-digit replica numbers (the longest replica strings, 22 bytes at W = 19)"""
    eng, ora = make_pair(6)
    try:
        events = [(0, W.EV_KILL, 4, 0)]
        for r in range(3):
            step_both(eng, ora, events)
        check_all(eng, ora, KEYS64, R=1000, what="R=1000")
        with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
            eng.route(KEYS64, [0], 1001)
    finally:
        eng.close()


def test_thirteen_byte_addresses():
    """an explicit 13-byte address set: replica strings of 14 to 16 bytes"""
    n = 40
    addrs = S.addresses(n, 13, 0)
    assert all(len(a) == 13 for a in addrs)
    eng = swimsim.Cluster(n, addresses=addrs)
    try:
        ora = OracleSim(n, addresses=addrs)
        events = [(0, W.EV_KILL, 7, 0)]
        for r in range(3):
            step_both(eng, ora, events)
        check_all(eng, ora, KEYS64, addresses=addrs, what="W=13")
        check_all(eng, ora, KEYS64, R=1000, addresses=addrs, what="W=13 R=1000")
        a, ok = eng.node(3).Lookup(KEYS64[0])
        ring = OracleRing(100)
        st = ora.row(3)[0]
        ring.add_remove_servers([addrs[m] for m in range(n) if st[m] <= 1], [])
        assert (a, ok) == ring.lookup(KEYS64[0])
    finally:
        eng.close()


# ---- 2. a shared replica hash, the wrap-around, an empty ring --------------------------------------------------------

def test_collision_and_wrap():
    """N = 256, R = 100, converged, synthetic addresses: members 185 and 215 share replica hash 581480965, and
    "key-226936" (hash 581472960) falls just below it. With every member present the lower index 185 owns the point;
    rows that hold 185 faulty answer 215; rows that hold both faulty answer 97, the next point's owner. "wrap-8000"
    hashes above every point and wraps to the first point's owner, 122. The constants are what the oracle answers (the
    comparison below is against the oracle's rings, the constants only pin the scenario)."""
    n = 256
    keys = ["key-226936", "wrap-8000"] + KEYS64[:14]
    eng, ora = make_pair(n)
    try:
        want = check_all(eng, ora, keys, what="all present")
        assert (want[:, 0] == 185).all() and (want[:, 1] == 122).all()
        pts = _points(100, n)
        assert fingerprint32(b"wrap-8000") > max(h for h, _ in pts)
        assert sum(1 for h, _ in pts if h == 581480965) == 1           # one point for the two members' shared hash
        without_185 = [3, 64, 185, 255]
        without_both = [0, 63, 200]
        for o in without_185 + without_both:
            eng.set_member(o, 185, swimsim.FAULTY, swimsim.T0_MS)
            ora.set_member(o, 185, swimsim.FAULTY, swimsim.T0_MS)
        for o in without_both:
            eng.set_member(o, 215, swimsim.FAULTY, swimsim.T0_MS)
            ora.set_member(o, 215, swimsim.FAULTY, swimsim.T0_MS)
        want = check_all(eng, ora, keys, what="185 / 215 faulty in some rows")
        assert (want[without_185, 0] == 215).all() and (want[without_both, 0] == 97).all()
        rest = [o for o in range(n) if o not in without_185 + without_both]
        assert (want[rest, 0] == 185).all() and (want[:, 1] == 122).all()
        ag = metrics.route_agreement(*eng.route_census(keys, "all")[:4])
        assert ag.distinct[0] == 3 and ag.owner[0] == 185 and ag.count[0] == n - 7
    finally:
        eng.close()


def test_all_faulty_row_answers_minus_one():
    n = 70
    eng, ora = make_pair(n)
    try:
        for o in (5, 69):
            for m in range(n):
                eng.set_member(o, m, swimsim.FAULTY, swimsim.T0_MS)
                ora.set_member(o, m, swimsim.FAULTY, swimsim.T0_MS)
        want = check_all(eng, ora, KEYS64, what="rows 5 and 69 all faulty")
        assert (want[[5, 69]] == -1).all() and (want[[4, 6, 68]] >= 0).all()
        counted, off, own, cnt, _ = eng.route_census(KEYS64, "all")
        for k in range(len(KEYS64)):
            assert own[int(off[k])] == -1 and cnt[int(off[k])] == 2
        assert eng.node(5).Lookup(KEYS64[0]) == ("", False)
        a, ok = eng.node(4).Lookup(KEYS64[0])
        assert ok and a == swimsim.address_of(int(want[4, 0]))
    finally:
        eng.close()


def test_every_wave_and_both_list_bounds():
    """N = 4,200 (NP = 4,224 = 16.5 groups of 256 members): every wave of k_route streams groups, wave 0 takes a second
    step, and the last group is half full. 300 keys: a second step of the key loop, the last one partly filled. The
    rows are converged except: rows holding 6 scattered members (the direct path in mode 0: 6 * 6 * 100 <= 4,200),
    7 members (just past the switch point), 512 members (exactly the list's capacity: direct in mode 2) and 513 (one
    more: the walk in every mode), and a few rows that miss members at the group edges."""
    n = 4200
    keys = [f"k{i}" for i in range(300)]
    eng, ora = make_pair(n)
    try:
        rng = np.random.default_rng(3)
        sparse = {11: [3, 255, 256, 1027, 4097, 4199], 4199: [0, 63, 64, 2048, 4095, 4096, 4198],
                  256: sorted(rng.choice(n, 512, replace=False)), 1023: sorted(rng.choice(n, 513, replace=False))}
        for o, present in sparse.items():
            st = np.full(n, swimsim.FAULTY, np.uint8)
            st[present] = swimsim.ALIVE
            st[present[0]] = swimsim.SUSPECT
            eng.set_row(o, st, np.full(n, swimsim.T0_MS, np.int64))
            for m in range(n):
                ora.set_member(o, m, int(st[m]), swimsim.T0_MS)
        for o, gone in {0: [0, 255, 256], 2100: [4096, 4199], 4100: [1023, 1024, 4095]}.items():
            for m in gone:
                eng.set_member(o, m, swimsim.TOMBSTONE, swimsim.T0_MS)
                ora.set_member(o, m, swimsim.TOMBSTONE, swimsim.T0_MS)
        eng.set_live(1023, False)
        ora.set_live(1023, False)
        want = check_all(eng, ora, keys, what="n=4200")
        assert len(np.unique(want)) > 250
    finally:
        eng.close()


# ---- 3. histograms: buffers, chunked passes, shards -----------------------------------------------------------------

def mid_cascade(shards=0):
    """the cascade after round 30: about half of the live nodes have dropped the killed members"""
    wl = W.config3(n=300, rounds=40, kill_round=3)
    eng, ora = make_pair(wl.n, shards=shards)
    eng.step(31, wl.events)
    ora.run(31, wl.events)
    return eng, ora, cascade_keys(wl)


def test_small_cap_returns_the_full_size_and_complete_offsets():
    eng, ora, keys = mid_cascade()
    try:
        want = expected_hist(oracle_owners(ora, keys), live_mask(ora, "live"))
        assert len(want[2]) > len(keys), "some key has more than one owner"
        L = swimsim.load_library()
        blob, koff = swimsim._pack_keys(keys)
        K = len(keys)
        for cap in (0, 1, K, len(want[2]) - 1, len(want[2])):
            hoff = np.full(K + 1, 77, np.uint64)
            own = np.full(max(1, cap) + 1, -9, np.int32)
            cnt = np.full(max(1, cap) + 1, 9, np.uint32)
            counted, nh = C.c_uint32(), C.c_size_t()
            rc = L.swimsim_route_census(eng.h, blob, koff.ctypes.data, K, 100, 0, 0, C.byref(counted), hoff.ctypes.data,
                                        own.ctypes.data if cap else None, cnt.ctypes.data if cap else None, cap,
                                        C.byref(nh), None)
            assert rc == 0 and nh.value == len(want[2]) and counted.value == want[0]
            assert (hoff == want[1]).all()
            assert (own[:cap] == want[2][:cap]).all() and (cnt[:cap] == want[3][:cap]).all()
            assert (own[cap:] == -9).all() and (cnt[cap:] == 9).all()     # nothing past cap is written
    finally:
        eng.close()


def test_full_exception_buffer_reruns_over_fewer_keys():
    """SWIMSIM_ROUTE_EXC_CAP (read when the census scratch is first allocated) bounds the exception pairs of a pass;
    the engine never goes below one pair per row (300 here). Mid-cascade the 64 keys have more exceptions than that, so
    the pass overflows and is run again over key chunks; the result is the same."""
    eng, ora, keys = mid_cascade()
    os.environ["SWIMSIM_ROUTE_EXC_CAP"] = "1"
    try:
        owners = oracle_owners(ora, keys)
        for who in ("live", "all"):
            mask = live_mask(ora, who)
            first = int(np.nonzero(mask)[0][0])
            exceptions = int((owners[mask] != owners[first]).sum())
            assert exceptions > 300, f"{exceptions} exception pairs do not overflow a buffer of 300"
            for mode in MODES:
                check_hist(eng.route_census(keys, who, 100, mode), expected_hist(owners, mask), f"chunked {who} {mode}")
    finally:
        del os.environ["SWIMSIM_ROUTE_EXC_CAP"]
        eng.close()


@pytest.mark.parametrize("call, nkeys, n", [("route_census", 90000, 1), ("replica_census", 30000, 2)])
def test_more_runs_than_the_first_read_back(call, nkeys, n):
    """The census reads the first 65,536 runs of a pass back together with their number and the rest with a second
    copy. 64 members, converged, except row 5, which holds only six of them: with the buffer raised to 262,144 pairs
    one pass holds every pair, and row 5 alone differs from the base (row 0) in more than 65,536 runs: a run is a
    (key, owner != base owner) entry for route_census (81,586 of the 90,000 keys), a member of the symmetric difference
    of the two sets for replica_census (108,880 for 30,000 keys at n = 2). The expectation is built from two oracle
    rings, the 64 members' and the six members': every other row counts for the first, row 5 for the second."""
    N, R, six = 64, 100, [3, 17, 22, 40, 41, 63]
    keys = [f"k{i}" for i in range(nkeys)]
    eng, ora = make_pair(N)
    os.environ["SWIMSIM_ROUTE_EXC_CAP"] = "262144"
    try:
        st = np.full(N, swimsim.FAULTY, np.uint8)
        st[six] = swimsim.ALIVE
        eng.set_row(5, st, np.full(N, swimsim.T0_MS, np.int64))
        for m in range(N):
            ora.set_member(5, m, int(st[m]), swimsim.T0_MS)
        ost, _ = ora.rows()
        assert all(ora.live(o) for o in range(N))
        assert (np.delete(ost, 5, axis=0) == swimsim.ALIVE).all() and list(np.nonzero(ost[5] <= 1)[0]) == six
        addr = [swimsim.address_of(m) for m in range(N)]
        index = {a: m for m, a in enumerate(addr)}
        sets = []                                                     # [K, n] member indices under the two rings
        for members in (range(N), six):
            ring = OracleRing(R)
            ring.add_remove_servers([addr[m] for m in members], [])
            got = [[index[ring.lookup(key)[0]]] for key in keys] if call == "route_census" else \
                  [[index[a] for a in ring.lookup_n(key, n)] for key in keys]
            sets.append(np.array(got, np.int64))
            assert sets[-1].shape == (nkeys, n)
        # entries (key, member, rows): N - 1 rows answer the first ring's members, one row the second's; equal ones add
        code = np.concatenate([(np.arange(nkeys)[:, None] * N + s).ravel() for s in sets])
        rows = np.concatenate([np.full(nkeys * n, N - 1), np.full(nkeys * n, 1)])
        u, inv = np.unique(code, return_inverse=True)                 # ascending by (key, member)
        cnt = np.bincount(inv.ravel(), weights=rows).astype(np.uint32)
        off = np.searchsorted(u // N, np.arange(nkeys + 1)).astype(np.uint64)
        runs = int((sets[0] != sets[1]).sum()) if call == "route_census" else int((cnt != N).sum())
        assert 65536 < runs < 262144, f"{runs} exception runs"
        got = eng.route_census(keys, "live", R, 0) if call == "route_census" else eng.replica_census(keys, n, "live", R, 0)
        check_hist(got, (N, off, (u % N).astype(np.int32), cnt), f"{call} with {runs} runs", per_key=N * n)
    finally:
        del os.environ["SWIMSIM_ROUTE_EXC_CAP"]
        eng.close()


def test_sharded_equals_unsharded():
    """ShardedCluster(300, 3): route goes to the owning shards, histograms add per (key, owner)"""
    eng, ora, keys = mid_cascade(shards=3)
    one, _, _ = mid_cascade()
    try:
        want = check_all(eng, ora, keys, what="sharded")
        obs = [299, 0, 100, 99, 200, 199, 100]                        # unordered, across the shards, a duplicate
        assert (eng.route(keys, obs) == want[obs]).all()
        for who in ("live", "all"):
            a, b = eng.route_census(keys, who), one.route_census(keys, who)
            assert a[0] == b[0] and all((x == y).all() for x, y in zip(a[1:4], b[1:4]))
        # a shard alone counts its own rows
        part = eng.shards[1].route_census(keys, "all")
        check_hist(part, expected_hist(want[100:200], np.ones(100, bool)), "shard 1")
        with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
            eng.shards[1].route(keys, [99])                         # not a row of this handle
    finally:
        eng.close()
        one.close()


# ---- 4. non-interference, memory, errors ----------------------------------------------------------------------------

def test_routing_changes_nothing():
    """digest(), checksums() and memory() are equal before and after the calls and the next 5 rounds still match the
    oracle. The first call of a handle allocates the point table and the scratch (swimsim.h: on first use, kept until
    destroy), which shows in memory()'s total only; every later call leaves memory() as it is."""
    wl = W.config3(n=300, rounds=40, kill_round=3)
    keys = cascade_keys(wl)
    eng, ora = make_pair(wl.n)
    try:
        eng.step(30, wl.events)
        ora.run(30, wl.events)
        before = (eng.digest(), eng.checksums().copy(), eng.memory(), eng.counters())
        eng.route(keys, list(range(300)))
        eng.route_census(keys, "live")
        first = eng.memory()
        assert first["total"] > before[2]["total"]
        assert {k: v for k, v in first.items() if k != "total"} == {k: v for k, v in before[2].items() if k != "total"}
        for mode in MODES:
            eng.route(keys, list(range(300)), 100, mode)
            eng.route_census(keys, "live", 100, mode)
            eng.route_census(keys, "all", 100, mode)
        assert eng.memory() == first
        assert eng.digest() == before[0] and (eng.checksums() == before[1]).all() and eng.counters() == before[3]
        assert eng.digest() == ora.digest() and (eng.checksums() == ora.checksums()).all()
        for r in range(5):
            step_both(eng, ora, wl.events)
            assert (eng.checksums() == ora.checksums()).all() and eng.digest() == ora.digest(), f"round {30 + r}"
        assert eng.counters() == ora.counters()
        check_all(eng, ora, keys[:8], what="after 5 more rounds", modes=(0,))
    finally:
        eng.close()


def test_a_handle_that_never_routes_holds_what_it_held():
    a, b = swimsim.Cluster(300), swimsim.Cluster(300)
    try:
        a.step(2)
        b.step(2)
        b.route(KEYS64, [1])
        b.route_census(KEYS64)
        ma, mb = a.memory(), b.memory()
        assert mb["total"] > ma["total"]
        assert {k: v for k, v in ma.items() if k != "total"} == {k: v for k, v in mb.items() if k != "total"}
    finally:
        a.close()
        b.close()


def test_errors_leave_the_next_call_correct():
    n = 40
    eng, ora = make_pair(n)
    try:
        events = [(0, W.EV_KILL, 4, 0)]
        eng.step(4, events)
        ora.run(4, events)
        L = swimsim.load_library()
        blob, koff = swimsim._pack_keys(KEYS64)
        K = len(KEYS64)
        obs = np.arange(n, dtype=np.uint32)
        out = np.full((n, K), -7, np.int32)
        hoff = np.full(K + 1, 77, np.uint64)
        own = np.full(4 * K, -9, np.int32)
        cnt = np.full(4 * K, 9, np.uint32)
        counted, nh = C.c_uint32(123), C.c_size_t(456)

        def route(keys=blob, off=koff.ctypes.data, nkeys=K, R=100, observers=obs.ctypes.data, nobs=n, mode=0,
                  owners=out.ctypes.data):
            return L.swimsim_route(eng.h, keys, off, nkeys, R, observers, nobs, mode, owners, None)

        def census(keys=blob, off=koff.ctypes.data, nkeys=K, R=100, who=0, mode=0, hist_off=hoff.ctypes.data):
            return L.swimsim_route_census(eng.h, keys, off, nkeys, R, who, mode, C.byref(counted), hist_off,
                                          own.ctypes.data, cnt.ctypes.data, len(own), C.byref(nh), None)

        assert route(keys=None) == -1 and route(off=None) == -1 and route(owners=None) == -1
        assert route(nkeys=0) == -1 and route(R=0) == -1 and route(R=1001) == -1
        assert route(observers=None) == -1 and route(nobs=0) == -1
        assert route(mode=3) == -1 and route(mode=-1) == -1
        bad = obs.copy()
        bad[7] = n
        assert route(observers=bad.ctypes.data) == -1
        assert (out == -7).all()
        assert census(keys=None) == -1 and census(off=None) == -1 and census(hist_off=None) == -1
        assert census(nkeys=0) == -1 and census(R=0) == -1 and census(R=1001) == -1
        assert census(who=2) == -1 and census(who=-1) == -1 and census(mode=3) == -1
        assert (hoff == 77).all() and (own == -9).all() and (cnt == 9).all() and counted.value == 123 and nh.value == 456
        with pytest.raises(ValueError):
            eng.route_census(KEYS64, "dead")
        with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
            eng.route(KEYS64, [])
        with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
            eng.route([], [0])
        check_all(eng, ora, KEYS64, what="after the errors")
        # keys of every FarmHash length path, the empty key included, and bytes keys
        odd = ["", "a", "abcd", "abcde", "twelve-bytes", "thirteen-byte", "x" * 24, "y" * 25, "z" * 300, b"\xff\x00\x80raw"]
        check_all(eng, ora, odd, what="odd keys")
    finally:
        eng.close()
