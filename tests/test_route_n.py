"""Replica sets through every node's own ring view (swimsim_route_n, swimsim_replica_census) against the CPU oracle.

Every expected value comes from the oracle alone, as in test_route.py: OracleSim.rows() and live() give the views, one
fresh OracleRing(R).add_remove_servers(...) is built per distinct set of members a row holds alive or suspect, and
OracleRing.lookup_n(key, n) answers every key, mapped to member indices. The ORDERED lists and the server counts of
every row and key are compared in modes 0 (automatic), 1 (ring walk) and 2 (direct path wherever the row fits the list);
the census is compared, for who = live and all, with a numpy count over those lists. Constants quoted in a test only pin
its scenario (they are what the oracle answers); the equality is against the oracle.
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
from test_route import KEYS64, MODES, answers_of, cascade_keys, live_mask, mid_cascade

pytestmark = pytest.mark.gpu


def oracle_prefs(ora, keys, n, R=100, addresses=None, rows=None):
    """(prefs[rows, K, n] int32 with -1 past the list, servers[rows]) of the oracle's state, every row by default"""
    addr = list(addresses) if addresses is not None else [swimsim.address_of(m) for m in range(ora.n)]
    index = {a: m for m, a in enumerate(addr)}
    ost, _ = ora.rows()
    rows = list(range(ora.n)) if rows is None else list(rows)
    out = np.full((len(rows), len(keys), n), -1, np.int32)
    srv = np.zeros(len(rows), np.uint32)
    views = answers_of(("prefs", n), R, addr if addresses is not None else ora.n, keys)   # (kept for the session)
    for j, o in enumerate(rows):
        present = ost[o] <= 1
        view = present.tobytes()
        if view not in views:
            ring = OracleRing(R)
            ring.add_remove_servers([addr[m] for m in np.nonzero(present)[0]], [])
            v = np.full((len(keys), n), -1, np.int32)
            for k, key in enumerate(keys):
                got = [index[a] for a in ring.lookup_n(key, n)]
                assert len(got) == min(n, int(present.sum())) and len(set(got)) == len(got)
                v[k, :len(got)] = got
            views[view] = (v, int(present.sum()))
        out[j], srv[j] = views[view]
    return out, srv


def expected_hist(prefs, mask):
    """(counted, hist_off, hist_member, hist_count) of the rows in mask: a numpy count over the oracle's lists"""
    off, mem, cnt = [0], [], []
    for k in range(prefs.shape[1]):
        v = prefs[mask, k].ravel()
        u, c = np.unique(v[v >= 0], return_counts=True)
        mem += list(u)
        cnt += list(c)
        off.append(len(mem))
    return int(mask.sum()), np.array(off, np.uint64), np.array(mem, np.int32), np.array(cnt, np.uint32)


def check_hist(got, want, srv, mask, n, what):
    counted, off, mem, cnt = got[:4]
    assert counted == want[0], f"{what}: counted {counted}, oracle {want[0]}"
    assert (off == want[1]).all(), f"{what}: hist_off differs at key {np.nonzero(off != want[1])[0][:3]}"
    assert len(mem) == len(want[2]) and (mem == want[2]).all() and (cnt == want[3]).all(), f"{what}: histogram entries differ"
    total = int(np.minimum(srv[mask].astype(np.int64), n).sum())     # the sum over the counted rows of min(n, cnt(row))
    for k in range(len(off) - 1):
        c = cnt[int(off[k]):int(off[k + 1])]
        assert int(c.sum()) == total and (c >= 1).all() and (c <= counted).all()
    assert got[4] >= 0


def check_lists(got, gsrv, want, srv, keys, what):
    assert got.shape == want.shape and got.dtype == np.int32 and gsrv.dtype == np.uint32
    assert (gsrv == srv).all(), f"{what}: servers differ at rows {np.nonzero(gsrv != srv)[0][:5]}"
    bad = np.argwhere((got != want).any(axis=2))
    assert not len(bad), (f"{what}: row {bad[0][0]} key {keys[bad[0][1]]!r}: engine {got[bad[0][0], bad[0][1]]} oracle "
                          f"{want[bad[0][0], bad[0][1]]} ({len(bad)} lists differ)")


def check_all(eng, ora, keys, ns=(3,), R=100, addresses=None, what="", modes=MODES, census=True):
    """route_n of every observer, and replica_census with live and all, for every n and mode; {n: oracle lists}"""
    res = {}
    for n in ns:
        want, srv = oracle_prefs(ora, keys, n, R, addresses)
        hists = {who: (live_mask(ora, who), expected_hist(want, live_mask(ora, who))) for who in ("live", "all") if census}
        for mode in modes:
            got, gsrv = eng.route_n(keys, list(range(ora.n)), n, R, mode)
            check_lists(got, gsrv, want, srv, keys, f"{what} n {n} mode {mode}")
            for who, (mask, hist) in hists.items():
                check_hist(eng.replica_census(keys, n, who, R, mode), hist, srv, mask, n, f"{what} n {n} mode {mode} who={who}")
        res[n] = want
    return res


def set_sparse_rows(eng, ora, sparse):
    """rows whose only present members are the listed ones (the first suspect, the others alive)"""
    n = ora.n
    for o, present in sparse.items():
        st = np.full(n, swimsim.FAULTY, np.uint8)
        st[list(present)] = swimsim.ALIVE
        st[list(present)[0]] = swimsim.SUSPECT
        eng.set_row(o, st, np.full(n, swimsim.T0_MS, np.int64))
        for m in range(n):
            ora.set_member(o, m, int(st[m]), swimsim.T0_MS)


# ---- 1. the cascade ---------------------------------------------------------------------------------------------------

def test_cascade():
    """W.config3(n=300, kill_round=3) as test_route.test_cascade: after round 2 every view is the same ring; after round
    30 about half of the live nodes have dropped the killed members, whose places in the replica sets go to the next
    owners; after round 39 the live nodes agree again. n = 1 is Lookup: it must equal eng.route of the same state."""
    wl = W.config3(n=300, rounds=40, kill_round=3)
    keys = cascade_keys(wl)
    eng, ora = make_pair(wl.n)
    try:
        agreed = {}
        for r in range(40):
            step_both(eng, ora, wl.events)
            if r in (2, 30, 39):
                want = check_all(eng, ora, keys, ns=(1, 3, 16), what=f"round {r}")
                assert (want[1][:, :, 0] == eng.route(keys, list(range(wl.n)))).all(), f"round {r}: n = 1 is not Lookup"
                c = eng.replica_census(keys, 3, "live")
                ag = metrics.replica_agreement(*c[:4], 3)
                sets = np.sort(want[3][live_mask(ora, "live")], axis=2)
                assert (ag.agreed == (sets == sets[0]).all(axis=(0, 2))).all()
                agreed[r] = int(ag.agreed.sum())
        assert agreed[2] == len(keys) and agreed[30] < len(keys) and agreed[39] == len(keys), agreed
        assert (eng.checksums() == ora.checksums()).all() and eng.digest() == ora.digest()
    finally:
        eng.close()


# ---- 2. a shared replica hash ------------------------------------------------------------------------------------------

SHARED_KEYS = ["key-226936", "key-806", "key-2920", "wrap-8000"]


def test_shared_hash_is_one_point():
    """N = 256, R = 100, synthetic addresses: members 185 and 215 share replica hash 581480965 and "key-226936" hashes
    just below it. The tree holds one node for the hash, 185's: 215's replica is no point of a view that holds both, and
    a walk that takes it lists 215 where the ring lists the next owner."""
    n = 256
    eng, ora = make_pair(n)
    try:
        want = check_all(eng, ora, SHARED_KEYS + KEYS64[:12], ns=(1, 2, 3, 5), what="all present")
        for k, lst in {1: [185], 2: [185, 97], 3: [185, 97, 55], 5: [185, 97, 55, 130, 107]}.items():
            assert (want[k][:, 0] == lst).all(), (k, want[k][0, 0])
        rows = {10: [55, 97, 185, 215], 20: [97, 185, 215], 30: [97, 215]}
        set_sparse_rows(eng, ora, rows)
        want = check_all(eng, ora, SHARED_KEYS, ns=(2, 3), what="sparse rows")
        assert list(want[2][10, 1]) == [185, 97] and list(want[3][10, 1]) == [185, 97, 55]      # key-806
        assert list(want[3][10, 2]) == [55, 185, 97]                                              # key-2920
        assert list(want[2][30, 0]) == [97, 215] and list(want[3][30, 0]) == [97, 215, -1]        # cnt = 2: ascending
        assert set(want[3][20, 0]) == {97, 185, 215}                                              # cnt = 3 = n
    finally:
        eng.close()


def collected_then_shared_cases(n=4200, R=100, nkeys=60000, most=6):
    """[(a, b, c, keys)]: present members a < b share a replica hash H, and the keys hash into the gap just before a's
    previous point p (in the view {a, b, c}), with no point of b or c between p and H and c's next point after H before
    b's. The walk from such a key collects a at p and then meets H: a's point, with b's duplicate entry behind it. A walk
    that takes that entry answers [a, b] for n = 2; the ring's next distinct owner is c."""
    hm = np.array([[fingerprint32(f"{swimsim.address_of(m)}{i}".encode()) for i in range(R)] for m in range(n)], np.int64)
    flat = hm.ravel()
    order = np.argsort(flat, kind="stable")
    at = np.nonzero(flat[order][1:] == flat[order][:-1])[0]
    pairs = [(int(order[i] // R), int(order[i + 1] // R), int(flat[order[i]])) for i in at if order[i] // R != order[i + 1] // R]
    kh = np.array([fingerprint32(f"key-{i}".encode()) for i in range(nkeys)], np.int64)
    cases = []
    for a, b, H in pairs:
        below = hm[a][hm[a] < H]
        if not len(below):
            continue
        p = int(below.max())
        if ((hm[b] > p) & (hm[b] < H)).any():
            continue
        for c in range(n):
            hc = hm[c]
            if c in (a, b) or ((hc > p) & (hc < H)).any() or not (hc > H).any():
                continue
            nb = hm[b][hm[b] > H]
            if len(nb) and nb.min() < hc[hc > H].min():
                continue
            view = np.concatenate([hm[a], hm[b], hc])
            lo = view[view < p]
            ks = np.nonzero((kh > (int(lo.max()) if len(lo) else -1)) & (kh <= p))[0][:2]
            if len(ks):
                cases.append((a, b, c, [f"key-{i}" for i in ks]))
                break
        if len(cases) == most:
            break
    return len(pairs), cases


def test_shared_hash_after_the_lower_member_was_collected():
    """The other duplicate shape: the lower member of a shared hash was collected at an earlier point, so a minimum
    over uncollected members (or a walk that only skips collected members) takes the higher member's duplicate entry
    for a real point. The pair 185 / 215 of N = 256 has no such key; N = 4,200 (420,000 points) is searched for pairs
    that do. Every case found is a row {a, b, c} routed with n = 2 in every mode; the ring answers [a, c]."""
    n = 4200
    npairs, cases = collected_then_shared_cases(n)
    assert npairs >= 5, "the synthetic addresses of 4,200 members share some replica hashes"
    assert cases, f"none of the {npairs} shared hashes has a key of this shape"
    eng, ora = make_pair(n)
    try:
        rows = {100 + 7 * j: sorted((a, b, c)) for j, (a, b, c, _) in enumerate(cases)}
        set_sparse_rows(eng, ora, rows)
        keys = [k for case in cases for k in case[3]]
        obs = list(rows)
        want, srv = oracle_prefs(ora, keys, 2, rows=obs)
        at = 0
        for j, (a, b, c, ks) in enumerate(cases):
            for _ in ks:
                assert list(want[j, at]) == [a, c], (a, b, c, keys[at], want[j, at])
                at += 1
        for mode in MODES:
            got, gsrv = eng.route_n(keys, obs, 2, 100, mode)
            check_lists(got, gsrv, want, srv, keys, f"collected-then-shared mode {mode}")
    finally:
        eng.close()


# ---- 3. small and sparse views ------------------------------------------------------------------------------------------

def test_self_only_start():
    """n = 65, every node knows itself and members 0 and 1: views of 1 to 3 servers against n = 3 and n = 16, so every
    list is the cnt <= n rule's: all servers in ascending member index"""
    (eng, ora), events, rounds = scenario_self_only()
    try:
        want = check_all(eng, ora, KEYS64[:20], ns=(3, 16), what="before round 0")
        lists = [row[row >= 0] for row in want[16][:, 0]]
        assert {len(x) for x in lists} == {2, 3} and all((np.diff(x) > 0).all() for x in lists)
        for r in range(rounds):
            step_both(eng, ora, events)
            check_all(eng, ora, KEYS64[:20], ns=(3, 16), what=f"round {r}")
        check_all(eng, ora, KEYS64[:9], ns=(2,), R=1, what="R=1")
    finally:
        eng.close()
    eng, ora = make_pair(5, init="self")                              # every view is the node itself: cnt = 1
    try:
        want = check_all(eng, ora, KEYS64[:5], ns=(1, 3), what="self only")
        assert (want[3][:, :, 0] == np.arange(5)[:, None]).all() and (want[3][:, :, 1:] == -1).all()
    finally:
        eng.close()


def test_single_node():
    eng, ora = make_pair(1)
    try:
        step_both(eng, ora, [])
        want = check_all(eng, ora, KEYS64[:5], ns=(1, 2), what="n=1")
        assert (want[1] == 0).all() and (want[2][:, :, 1] == -1).all()
        assert eng.node(0).LookupN(KEYS64[0], 3) == [swimsim.address_of(0)]
    finally:
        eng.close()


def test_one_replica_point_three_nodes():
    """R = 1 with N = 3: three points, most keys wrap to the first"""
    eng, ora = make_pair(3)
    try:
        events = [(1, W.EV_KILL, 2, 0)]
        for r in range(4):
            step_both(eng, ora, events)
            check_all(eng, ora, KEYS64, ns=(1, 2, 3), R=1, what=f"R=1 round {r}")
    finally:
        eng.close()


def test_all_faulty_row_lists_nothing():
    n = 70
    eng, ora = make_pair(n)
    try:
        for o in (5, 69):
            for m in range(n):
                eng.set_member(o, m, swimsim.FAULTY, swimsim.T0_MS)
                ora.set_member(o, m, swimsim.FAULTY, swimsim.T0_MS)
        want = check_all(eng, ora, KEYS64, ns=(3,), what="rows 5 and 69 all faulty")
        assert (want[3][[5, 69]] == -1).all() and (want[3][[4, 6, 68]] >= 0).all()
        prefs, srv = eng.route_n(KEYS64, [5, 4, 69], 3)
        assert list(srv) == [0, n, 0] and (prefs[[0, 2]] == -1).all()
        counted, off, mem, cnt, _ = eng.replica_census(KEYS64, 3, "all")
        assert counted == n and (mem >= 0).all() and cnt.max() == n - 2          # the empty views add nothing
        assert eng.node(5).LookupN(KEYS64[0], 3) == []
        assert eng.node(4).LookupN(KEYS64[0], 3) == [swimsim.address_of(int(m)) for m in want[3][4, 0]]
    finally:
        eng.close()


def test_eviction():
    """leave, tombstone and unknown (evicted) cells are not servers"""
    (eng, ora), events, rounds = scenario_eviction()
    try:
        seen = set()
        for r in range(rounds):
            step_both(eng, ora, events)
            if r in (2, 3, 5, 12, 31, 41, 42, 60):
                check_all(eng, ora, KEYS64[:32], ns=(3,), what=f"round {r}")
                seen |= set(np.unique(ora.rows()[0]))
        assert {3, 4, 7} <= seen, "the checked rounds show leave, tombstone and unknown cells"
    finally:
        eng.close()


# ---- 4. shapes ------------------------------------------------------------------------------------------------------------

def test_every_wave_and_both_list_bounds():
    """N = 4,200 and 300 keys with the rows of test_route.test_every_wave_and_both_list_bounds: 6 servers (direct in
    mode 0), 7 (past the switch point), 512 (the list's capacity: direct in mode 2) and 513 (the walk in every mode),
    and rows that miss members at the group edges. n = 16 makes the rows of 6 and 7 servers lists of all servers."""
    n = 4200
    keys = [f"k{i}" for i in range(300)]
    eng, ora = make_pair(n)
    try:
        rng = np.random.default_rng(3)
        set_sparse_rows(eng, ora, {11: [3, 255, 256, 1027, 4097, 4199], 4199: [0, 63, 64, 2048, 4095, 4096, 4198],
                                   256: sorted(rng.choice(n, 512, replace=False)), 1023: sorted(rng.choice(n, 513, replace=False))})
        for o, gone in {0: [0, 255, 256], 2100: [4096, 4199], 4100: [1023, 1024, 4095]}.items():
            for m in gone:
                eng.set_member(o, m, swimsim.TOMBSTONE, swimsim.T0_MS)
                ora.set_member(o, m, swimsim.TOMBSTONE, swimsim.T0_MS)
        eng.set_live(1023, False)
        ora.set_live(1023, False)
        want = check_all(eng, ora, keys, ns=(3, 16), what="n=4200")
        assert len(np.unique(want[3][:, :, 0])) > 250
    finally:
        eng.close()


def test_thousand_replica_points():
    eng, ora = make_pair(6)
    try:
        events = [(0, W.EV_KILL, 4, 0)]
        for r in range(3):
            step_both(eng, ora, events)
        check_all(eng, ora, KEYS64, ns=(3, 5), R=1000, what="R=1000")
        with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
            eng.route_n(KEYS64, [0], 3, 1001)
    finally:
        eng.close()


def test_thirteen_byte_addresses():
    n = 40
    addrs = S.addresses(n, 13, 0)
    eng = swimsim.Cluster(n, addresses=addrs)
    try:
        ora = OracleSim(n, addresses=addrs)
        events = [(0, W.EV_KILL, 7, 0)]
        for r in range(3):
            step_both(eng, ora, events)
        check_all(eng, ora, KEYS64, ns=(3, 16), addresses=addrs, what="W=13")
        ring = OracleRing(100)
        st = ora.row(3)[0]
        ring.add_remove_servers([addrs[m] for m in range(n) if st[m] <= 1], [])
        assert eng.node(3).LookupN(KEYS64[0], 3) == ring.lookup_n(KEYS64[0], 3)
    finally:
        eng.close()


# ---- 5. census mechanics ----------------------------------------------------------------------------------------------------

def test_small_cap_returns_the_full_size_and_complete_offsets():
    eng, ora, keys = mid_cascade()
    try:
        prefs, _ = oracle_prefs(ora, keys, 3)
        want = expected_hist(prefs, live_mask(ora, "live"))
        assert len(want[2]) > 3 * len(keys), "some key has more than n members over the rows"
        L = swimsim.load_library()
        blob, koff = swimsim._pack_keys(keys)
        K = len(keys)
        for cap in (0, 1, K, len(want[2]) - 1, len(want[2])):
            hoff = np.full(K + 1, 77, np.uint64)
            mem = np.full(max(1, cap) + 1, -9, np.int32)
            cnt = np.full(max(1, cap) + 1, 9, np.uint32)
            counted, nh = C.c_uint32(), C.c_size_t()
            rc = L.swimsim_replica_census(eng.h, blob, koff.ctypes.data, K, 100, 3, 0, 0, C.byref(counted), hoff.ctypes.data,
                                          mem.ctypes.data if cap else None, cnt.ctypes.data if cap else None, cap,
                                          C.byref(nh), None)
            assert rc == 0 and nh.value == len(want[2]) and counted.value == want[0]
            assert (hoff == want[1]).all()
            assert (mem[:cap] == want[2][:cap]).all() and (cnt[:cap] == want[3][:cap]).all()
            assert (mem[cap:] == -9).all() and (cnt[cap:] == 9).all()     # nothing past cap is written
    finally:
        eng.close()


def test_full_exception_buffer_reruns_over_fewer_keys():
    """SWIMSIM_ROUTE_EXC_CAP = 1 leaves the buffer at its floor, 2 * n * rows pairs (9,600 for n = 16 and 300 rows).
    Mid-cascade with n = 16, the keys below have more pairs than that (counted from the oracle's lists: per row and key,
    the members by which the row's set differs from the first counted row's), so the pass overflows and is run again
    over key chunks; the result is the same."""
    eng, ora, keys = mid_cascade()
    keys = keys + [f"key-{i}" for i in range(1000, 1400)]
    os.environ["SWIMSIM_ROUTE_EXC_CAP"] = "1"
    try:
        prefs, srv = oracle_prefs(ora, keys, 16)
        for who in ("live", "all"):
            mask = live_mask(ora, who)
            rows = np.nonzero(mask)[0]
            pairs = sum(len(set(prefs[o, k]) ^ set(prefs[rows[0], k])) for o in rows[1:] for k in range(len(keys)))
            assert pairs > 2 * 16 * 300, f"{pairs} pairs do not overflow a buffer of {2 * 16 * 300}"
            for mode in MODES:
                check_hist(eng.replica_census(keys, 16, who, 100, mode), expected_hist(prefs, mask), srv, mask, 16,
                           f"chunked {who} {mode}")
        # the route census of the same handle shares the buffer (now larger than its own floor) and answers as before
        one, _, _ = mid_cascade()
        try:
            a, b = eng.route_census(keys[:64], "live"), one.route_census(keys[:64], "live")
            assert a[0] == b[0] and all((x == y).all() for x, y in zip(a[1:4], b[1:4]))
        finally:
            one.close()
    finally:
        del os.environ["SWIMSIM_ROUTE_EXC_CAP"]
        eng.close()


def test_sharded_equals_unsharded():
    """ShardedCluster(300, 3): route_n goes to the owning shards, histograms add per (key, member)"""
    eng, ora, keys = mid_cascade(shards=3)
    one, _, _ = mid_cascade()
    try:
        want = check_all(eng, ora, keys, ns=(3,), what="sharded", modes=(0,))[3]
        obs = [299, 0, 100, 99, 200, 199, 100]                        # unordered, across the shards, a duplicate
        prefs, srv = eng.route_n(keys, obs, 3)
        assert (prefs == want[obs]).all() and (srv == one.route_n(keys, obs, 3)[1]).all()
        for who in ("live", "all"):
            a, b = eng.replica_census(keys, 3, who), one.replica_census(keys, 3, who)
            assert a[0] == b[0] and all((x == y).all() for x, y in zip(a[1:4], b[1:4]))
        part = eng.shards[1].replica_census(keys, 3, "all")           # a shard alone counts its own rows
        _, srv_all = oracle_prefs(ora, keys[:1], 3)
        check_hist(part, expected_hist(want[100:200], np.ones(100, bool)), srv_all[100:200], np.ones(100, bool), 3, "shard 1")
        with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
            eng.shards[1].route_n(keys, [99], 3)                    # not a row of this handle
    finally:
        eng.close()
        one.close()


# ---- 6. non-interference, memory, errors ------------------------------------------------------------------------------------

def test_replica_calls_change_nothing():
    """digest(), checksums(), counters() and memory() (apart from total at the first use) are equal before and after the
    calls, the next 5 rounds still match the oracle, and route / route_census, which share the point table and the
    scratch, answer what they answered before."""
    wl = W.config3(n=300, rounds=40, kill_round=3)
    keys = cascade_keys(wl)
    eng, ora = make_pair(wl.n)
    try:
        eng.step(30, wl.events)
        ora.run(30, wl.events)
        before = (eng.digest(), eng.checksums().copy(), eng.memory(), eng.counters())
        owners = eng.route(keys, list(range(300)))
        hist = eng.route_census(keys, "live")
        mem0 = eng.memory()
        eng.route_n(keys, list(range(300)), 16)
        eng.replica_census(keys, 16, "live")
        first = eng.memory()
        assert first["total"] > mem0["total"] > before[2]["total"]
        assert {k: v for k, v in first.items() if k != "total"} == {k: v for k, v in before[2].items() if k != "total"}
        for mode in MODES:
            for n in (1, 3, 16):
                eng.route_n(keys, list(range(300)), n, 100, mode)
                eng.replica_census(keys, n, "live", 100, mode)
                eng.replica_census(keys, n, "all", 100, mode)
        assert eng.memory() == first
        assert (eng.route(keys, list(range(300))) == owners).all()
        again = eng.route_census(keys, "live")
        assert again[0] == hist[0] and all((x == y).all() for x, y in zip(again[1:4], hist[1:4]))
        assert eng.memory() == first
        assert eng.digest() == before[0] and (eng.checksums() == before[1]).all() and eng.counters() == before[3]
        assert eng.digest() == ora.digest() and (eng.checksums() == ora.checksums()).all()
        for r in range(5):
            step_both(eng, ora, wl.events)
            assert (eng.checksums() == ora.checksums()).all() and eng.digest() == ora.digest(), f"round {30 + r}"
        assert eng.counters() == ora.counters()
        check_all(eng, ora, keys[:8], ns=(3,), what="after 5 more rounds", modes=(0,))
    finally:
        eng.close()


def test_a_handle_that_never_calls_them_holds_what_it_held():
    a, b = swimsim.Cluster(300), swimsim.Cluster(300)
    try:
        for c in (a, b):
            c.step(2)
            c.route(KEYS64, [1])
            c.route_census(KEYS64)
        b.route_n(KEYS64, [1], 3)
        b.replica_census(KEYS64, 3)
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
        out = np.full((n, K, 3), -7, np.int32)
        srv = np.full(n, 99, np.uint32)
        hoff = np.full(K + 1, 77, np.uint64)
        mem = np.full(8 * K, -9, np.int32)
        cnt = np.full(8 * K, 9, np.uint32)
        counted, nh = C.c_uint32(123), C.c_size_t(456)

        def route(keys=blob, off=koff.ctypes.data, nkeys=K, R=100, nn=3, observers=obs.ctypes.data, nobs=n, mode=0,
                  prefs=out.ctypes.data):
            return L.swimsim_route_n(eng.h, keys, off, nkeys, R, nn, observers, nobs, mode, prefs, srv.ctypes.data, None)

        def census(keys=blob, off=koff.ctypes.data, nkeys=K, R=100, nn=3, who=0, mode=0, hist_off=hoff.ctypes.data):
            return L.swimsim_replica_census(eng.h, keys, off, nkeys, R, nn, who, mode, C.byref(counted), hist_off,
                                            mem.ctypes.data, cnt.ctypes.data, len(mem), C.byref(nh), None)

        assert route(keys=None) == -1 and route(off=None) == -1 and route(prefs=None) == -1
        assert route(nkeys=0) == -1 and route(R=0) == -1 and route(R=1001) == -1
        assert route(nn=0) == -1 and route(nn=17) == -1
        assert route(observers=None) == -1 and route(nobs=0) == -1
        assert route(mode=3) == -1 and route(mode=-1) == -1
        bad = obs.copy()
        bad[7] = n
        assert route(observers=bad.ctypes.data) == -1
        assert L.swimsim_route_n(None, blob, koff.ctypes.data, K, 100, 3, obs.ctypes.data, n, 0, out.ctypes.data, None, None) == -1
        assert (out == -7).all() and (srv == 99).all()
        assert census(keys=None) == -1 and census(off=None) == -1 and census(hist_off=None) == -1
        assert census(nkeys=0) == -1 and census(R=0) == -1 and census(R=1001) == -1
        assert census(nn=0) == -1 and census(nn=17) == -1
        assert census(who=2) == -1 and census(who=-1) == -1 and census(mode=3) == -1
        assert (hoff == 77).all() and (mem == -9).all() and (cnt == 9).all() and counted.value == 123 and nh.value == 456
        with pytest.raises(ValueError):
            eng.replica_census(KEYS64, 3, "dead")
        for nn in (0, 17, -1, 2.5):
            with pytest.raises(ValueError):
                eng.route_n(KEYS64, [0], nn)
            with pytest.raises(ValueError):
                eng.replica_census(KEYS64, nn)
        with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
            eng.route_n(KEYS64, [], 3)
        with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
            eng.route_n([], [0], 3)
        assert route() == 0 and L.swimsim_route_n(eng.h, blob, koff.ctypes.data, K, 100, 3, obs.ctypes.data, n, 0,
                                                 out.ctypes.data, None, None) == 0         # servers may be NULL
        check_all(eng, ora, KEYS64, ns=(3, 16), what="after the errors")
        # keys of every FarmHash length path, the empty key included, and bytes keys
        odd = ["", "a", "abcd", "abcde", "twelve-bytes", "thirteen-byte", "x" * 24, "y" * 25, "z" * 300, b"\xff\x00\x80raw"]
        check_all(eng, ora, odd, ns=(3,), what="odd keys")
    finally:
        eng.close()
