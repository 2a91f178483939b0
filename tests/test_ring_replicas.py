"""Batched LookupN and groupReplicas on the device ring (include/swimring.h: swimring_lookup_n_batch,
swimring_group_replicas, swimring_last_replica_times; swimsim.ring.HashRing.lookup_n_ids / lookup_n_batch /
group_replicas).

The yardstick is the CPU oracle (oracle/ring_oracle.c through OracleRing). Its lookup_n walks the ring upwards
from the key's hash, so for n < server count its result is ordered; a CPU test pins that order against a walk
written here over OracleRing.points(). The GPU tests then ask for the same order from the device (the reference
itself returns a Go map, hashring.go:279-301, so the order is this project's guarantee), for set equality when
n >= server count, for cnt equal to the oracle's length and for -1 padding. Every comparison is exact and covers
every key.
"""
import bisect
import ctypes
import os
import random

import numpy as np
import pytest

from oracle_ffi import OracleRing, fingerprint32

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "ringpop-go_amd", "swimsim", "libswimsim.so")
LIST_MAX = 16            # csrc/swimring.hip LN_LIST_MAX: n above it uses the seen-bitmap instead of the LDS list


def walk(points, h, n):
    """hashring.go:279-301 / rbtree.go:262-286 over the sorted (hash, owner) points: from the first point with
    hash >= h, wrapping once, at most len(points) points, the first n distinct owners in order of occurrence"""
    P = len(points)
    if P == 0 or n == 0:
        return []
    start = bisect.bisect_left(points, (h, ""))
    if start == P:
        start = 0
    out = []
    for i in range(P):
        o = points[(start + i) % P][1]
        if o not in out:
            out.append(o)
            if len(out) == n:
                break
    return out


def addresses(host, count):
    return [f"10.0.{host}.{i // 250}:{3000 + i % 250}" for i in range(count)]


def length_keys():
    """key lengths 0, 1, 4, 5, 12, 13, 24, 25 and 60: every Fingerprint32 length path and its edges"""
    return ["x" * L for L in (0, 1, 4, 5, 12, 13, 24, 25, 60)] + [("ab" * 30)[:L] for L in (4, 12, 24, 25)]


# ------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------
def test_library_exports_the_replica_entry_points():
    lib = ctypes.CDLL(LIB)
    for name in ("swimring_lookup_n_batch", "swimring_group_replicas", "swimring_last_replica_times"):
        assert hasattr(lib, name), name


def test_null_handle_is_einval():
    lib = ctypes.CDLL(LIB)
    P, sz, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    lib.swimring_lookup_n_batch.restype = ctypes.c_int
    lib.swimring_lookup_n_batch.argtypes = [P, P, P, sz, u32, P, P]
    lib.swimring_group_replicas.restype = ctypes.c_int
    lib.swimring_group_replicas.argtypes = [P, P, P, sz, u32, P, P, P, P, P, P]
    off = (ctypes.c_uint64 * 2)(0, 1)
    out = (ctypes.c_int32 * 4)()
    cnt = (ctypes.c_uint32 * 4)()
    big = (ctypes.c_uint64 * 4)()
    nd = ctypes.c_size_t()
    assert lib.swimring_lookup_n_batch(None, b"k", off, 1, 3, out, cnt) == -1
    assert lib.swimring_group_replicas(None, b"k", off, 1, 3, out, cnt, out, big, cnt, ctypes.byref(nd)) == -1
    lib.swimring_last_replica_times.restype = ctypes.c_int
    lib.swimring_last_replica_times.argtypes = [P, P, P]
    assert lib.swimring_last_replica_times(None, None, None) == -1


def test_oracle_lookup_n_is_the_ordered_ring_walk():
    """pins the yardstick: OracleRing.lookup_n for n < server count is the walk above, in order"""
    o = OracleRing(10)
    o.add_remove_servers([f"server{i}" for i in range(10)])
    pts = o.points()
    for n in (1, 3, 7):
        for k in range(200):
            key = f"key-{k}"
            assert o.lookup_n(key, n) == walk(pts, fingerprint32(key.encode()), n), (key, n)


# ------------------------------------------------------------------------------------------
# GPU vs oracle
# ------------------------------------------------------------------------------------------
def _gpu_ring(R):
    from swimsim.ring import HashRing
    return HashRing(R, device=0)


def _check_rows(g, ids, cnt, want_rows, n, nservers):
    """ids / cnt against the oracle's per-key lists: ordered below the server count, as sets from it on"""
    assert ids.shape == (len(want_rows), n) and ids.dtype == np.int32
    assert cnt.shape == (len(want_rows),)
    names = {}
    for k, want in enumerate(want_rows):
        c = int(cnt[k])
        assert c == len(want), (k, c, len(want))
        got = [names.setdefault(int(i), g.name(int(i))) for i in ids[k, :c]]
        assert (ids[k, :c] >= 0).all()
        assert (ids[k, c:] == -1).all(), k
        if n < nservers:
            assert got == want, (k, n)
        else:
            assert len(set(got)) == len(got) and set(got) == set(want), (k, n)


def _check(g, o, keys, n):
    ids, cnt = g.lookup_n_ids(keys, n)
    _check_rows(g, ids, cnt, [o.lookup_n(k, n) for k in keys], n, o.server_count())
    return ids, cnt


@pytest.fixture(scope="module")
def ring300():
    """the 300-server, 100-replica ring and the oracle's n = 3 answers for 5,000 keys (50 of them duplicates),
    built once"""
    servers = addresses(7, 300)
    g, o = _gpu_ring(100), OracleRing(100)
    try:
        assert g.add_remove_servers(servers) and o.add_remove_servers(servers)
        keys = [f"key-{k}" for k in range(4950)]
        keys += keys[100:150]
        want3 = [o.lookup_n(k, 3) for k in keys]
        yield g, o, keys, want3
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_edges_empty_ring_n0_no_keys():
    g = _gpu_ring(10)
    try:
        keys = ["a", "b", ""]
        for _ in range(2):                       # a fresh ring, then a ring whose servers were all removed
            ids, cnt = g.lookup_n_ids(keys, 3)
            assert ids.shape == (3, 3) and (ids == -1).all() and (cnt == 0).all()
            assert g.lookup_n_batch(keys, 3) == [[], [], []]
            ids, cnt = g.lookup_n_ids(keys, 0)
            assert ids.shape == (3, 0) and cnt.shape == (3,) and (cnt == 0).all()
            ids, cnt = g.lookup_n_ids([], 3)
            assert ids.shape == (0, 3) and cnt.shape == (0,)
            by_key, by_dest = g.group_replicas(keys, 3)
            assert by_key == {0: [], 1: [], 2: []} and by_dest == {}
            assert g.group_replicas([], 3) == ({}, {})
            assert g.group_replicas(keys, 0) == ({0: [], 1: [], 2: []}, {})
            g.add_remove_servers(["server1", "server2", "server3"])
            ids, cnt = g.lookup_n_ids(keys, 0)   # n = 0 on a ring with servers
            assert ids.shape == (3, 0) and (cnt == 0).all()
            assert (g.lookup_n_ids(keys, 2)[1] == 2).all()
            g.add_remove_servers([], ["server1", "server2", "server3"])
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_oversize_matrix_and_null_arguments_are_einval():
    """nkeys * n beyond 2^31 - 1 entries is refused before anything is allocated or written; so are NULL outputs"""
    from swimsim.ring import _lib
    g = _gpu_ring(10)
    try:
        g.add_remove_servers(["server1", "server2", "server3"])
        L = _lib()
        off = np.array([0, 1, 2], np.uint64)
        out = np.full(8, 7, np.int32)
        cnt = np.full(2, 7, np.uint32)
        dest = np.full(3, 7, np.int32)
        doff = np.full(4, 7, np.uint64)
        kidx = np.full(8, 7, np.uint32)
        nd = ctypes.c_size_t(7)
        for n in (1 << 31, 0xffffffff, 1 << 30):
            assert L.swimring_lookup_n_batch(g.h, b"ab", off.ctypes.data, 2, n, out.ctypes.data, cnt.ctypes.data) == -1
            assert L.swimring_group_replicas(g.h, b"ab", off.ctypes.data, 2, n, out.ctypes.data, cnt.ctypes.data,
                                             dest.ctypes.data, doff.ctypes.data, kidx.ctypes.data, ctypes.byref(nd)) == -1
        assert L.swimring_lookup_n_batch(g.h, b"ab", off.ctypes.data, 2, 2, None, cnt.ctypes.data) == -1
        assert L.swimring_lookup_n_batch(g.h, b"ab", off.ctypes.data, 2, 2, out.ctypes.data, None) == -1
        assert L.swimring_lookup_n_batch(g.h, b"ab", None, 2, 2, out.ctypes.data, cnt.ctypes.data) == -1
        assert L.swimring_group_replicas(g.h, b"ab", off.ctypes.data, 2, 2, None, None, None, doff.ctypes.data,
                                         kidx.ctypes.data, ctypes.byref(nd)) == -1
        assert (out == 7).all() and (cnt == 7).all() and (kidx == 7).all() and (dest == 7).all()
        ids, c = g.lookup_n_ids(["a", "b"], 2)               # the handle is still usable
        assert (c == 2).all() and (ids >= 0).all()
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_tiny_ring_wraps_without_revisiting():
    """R = 1, 3 servers: P = 3 points, far below one 64-point step; keys hashing above the last point start at 0"""
    servers = ["server1", "server2", "server3"]
    g, o = _gpu_ring(1), OracleRing(1)
    try:
        g.add_remove_servers(servers)
        o.add_remove_servers(servers)
        pts = o.points()
        assert len(pts) == 3
        top = pts[-1][0]
        above = [f"wrap-{i}" for i in range(4000) if fingerprint32(f"wrap-{i}".encode()) > top][:8]
        assert len(above) == 8
        keys = above + [f"low-{i}" for i in range(12)] + [""]
        for n in (1, 2, 3, 5):
            ids, cnt = _check(g, o, keys, n)
            assert (cnt == min(n, 3)).all()
            for k in range(len(keys)):
                row = ids[k, :cnt[k]]
                assert len(set(row.tolist())) == len(row)
        for key in above:                        # the wrap: the first owner is the owner of point 0
            assert g.lookup_n_batch([key], 1) == [[pts[0][1]]]
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_equal_hash_starts_at_that_point():
    """key "server10" hashes like replica 0 of "server1": the bound is >=, so that point's owner comes first"""
    servers = ["server1", "server2", "server3", "server4"]
    g, o = _gpu_ring(10), OracleRing(10)
    try:
        g.add_remove_servers(servers)
        o.add_remove_servers(servers)
        hs, ow = g.points()
        h = fingerprint32(b"server10")
        at = [g.name(int(ow[i])) for i in range(len(hs)) if int(hs[i]) == h]
        assert len(at) == 1
        for n in (1, 2, 3):
            assert g.lookup_n_batch(["server10"], n)[0][0] == at[0]
            _check(g, o, ["server10", "server1", "server20"], n)
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_duplicates_inside_one_step():
    """2 servers x 100 replicas: every 64-point step is full of repeated owners"""
    g, o = _gpu_ring(100), OracleRing(100)
    try:
        g.add_remove_servers(["server1", "server2"])
        o.add_remove_servers(["server1", "server2"])
        keys = [f"dup-{k}" for k in range(500)]
        ids, _ = _check(g, o, keys, 1)
        assert (ids[:, 0] == g.lookup_ids(keys)).all()
        _check(g, o, keys, 2)
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, LIST_MAX, LIST_MAX + 1, 63, 64, 65, 299])
def test_gpu_wave_width_crossings(ring300, n):
    """n around the wave width, on both sides of the list / bitmap crossover, and n = server count - 1, which
    walks nearly the whole ring for every key; the ring itself must come out untouched"""
    g, o, _, _ = ring300
    keys = length_keys() + [f"cross-{k}" for k in range(70 - len(length_keys()))]
    assert len(keys) == 70
    before = [a.copy() for a in g.points()]
    _check(g, o, keys, n)
    after = g.points()
    assert (before[0] == after[0]).all() and (before[1] == after[1]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("nkeys", [1, 63, 64, 65, 5000])
def test_gpu_grid_tails(ring300, nkeys):
    g, o, keys, want3 = ring300
    keys, want3 = keys[:nkeys], want3[:nkeys]
    ids, cnt = g.lookup_n_ids(keys, 3)
    _check_rows(g, ids, cnt, want3, 3, o.server_count())
    rng = random.Random(nkeys)
    for k in rng.sample(range(nkeys), min(20, nkeys)):
        one, c1 = g.lookup_n_ids([keys[k]], 3)
        assert (one[0] == ids[k]).all() and c1[0] == cnt[k]
    first, c = g.lookup_n_ids(keys, 1)
    assert (c == 1).all() and (first[:, 0] == g.lookup_ids(keys)).all()
    assert (first[:, 0] == ids[:, 0]).all()


def churn_batches(servers, rounds, seed):
    """add / remove rounds: fresh adds, duplicate adds inside a call, removes of present and of absent servers"""
    rng = random.Random(seed)
    live = set()
    out = []
    for _ in range(rounds):
        add = rng.sample(servers, rng.randint(len(servers) // 8, len(servers) // 3))
        rem = rng.sample(sorted(live), min(len(live), rng.randint(1, len(servers) // 4))) if live else []
        rem += rng.sample(servers, 3)
        add += add[:2]
        live |= set(add)
        live -= set(rem)
        out.append((add, rem, set(live)))
    return out


@pytest.mark.gpu
def test_gpu_lookup_n_after_churn():
    servers = addresses(9, 2000)
    hashes = [fingerprint32(f"{s}{i}".encode()) for s in servers for i in range(100)]
    assert len(hashes) - len(set(hashes)) > 0    # the candidate set includes hash collisions
    g, o = _gpu_ring(100), OracleRing(100)
    try:
        for rnd, (add, rem, live) in enumerate(churn_batches(servers, 4, seed=23)):
            assert g.add_remove_servers(add, rem) == o.add_remove_servers(add, rem)
            assert g.server_count() == o.server_count() == len(live)
            for keys, n in (([f"churn-{rnd}-{k}" for k in range(1000)], 3), ([f"c17-{rnd}-{k}" for k in range(20)], 17)):
                ids, cnt = _check(g, o, keys, n)
                assert (cnt == n).all()
                assert {g.name(int(i)) for i in np.unique(ids)} <= live
    finally:
        g.close()


def _group_in_python(rows):
    """replicator.go:176-188 over per-key owner lists"""
    by_dest = {}
    for k, dests in enumerate(rows):
        for d in dests:
            by_dest.setdefault(d, []).append(k)
    return by_dest


@pytest.mark.gpu
def test_gpu_group_replicas(ring300):
    g, o, keys, want3 = ring300
    ids, cnt = g.lookup_n_ids(keys, 3)
    gids, gcnt, dest, doff, kidx = g.group_replica_ids(keys, 3)
    assert (gids == ids).all() and (gcnt == cnt).all()
    assert (np.diff(dest) > 0).all() and int(doff[0]) == 0 and (np.diff(doff.astype(np.int64)) > 0).all()
    assert len(kidx) == int(doff[-1]) == int(cnt.sum())
    by_key, by_dest = g.group_replicas(keys, 3)
    assert by_key == dict(enumerate(want3))
    want = _group_in_python(want3)
    assert by_dest == want                                   # ordered key lists per destination
    assert list(by_dest) == [g.name(int(d)) for d in dest]   # destinations ascending by server id
    assert sum(len(v) for v in by_dest.values()) == int(cnt.sum())
    for k in range(4950, 5000):                              # a duplicated key is two entries
        for d in want3[k]:
            assert k in by_dest[d] and k - 4850 in by_dest[d]


@pytest.mark.gpu
def test_gpu_group_replicas_every_server_and_empty_ring():
    servers = [f"server{i}" for i in range(5)]
    g, o = _gpu_ring(10), OracleRing(10)
    try:
        assert g.group_replicas(["a", "b"], 3) == ({0: [], 1: []}, {})
        _, _, dest, doff, kidx = g.group_replica_ids(["a", "b"], 3)
        assert len(dest) == 0 and list(doff) == [0] and len(kidx) == 0
        g.add_remove_servers(servers)
        o.add_remove_servers(servers)
        keys = [f"k{i}" for i in range(40)]
        for n in (5, 9):
            by_key, by_dest = g.group_replicas(keys, n)
            for k, key in enumerate(keys):
                assert sorted(by_key[k]) == sorted(o.lookup_n(key, n)) == sorted(servers)
            assert by_dest == {s: list(range(40)) for s in servers}
            ids, cnt, dest, doff, kidx = g.group_replica_ids(keys, n)
            assert (cnt == 5).all() and (ids[:, 5:] == -1).all() and len(kidx) == 200
            assert list(doff) == [0, 40, 80, 120, 160, 200]
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_replica_calls_leave_last_times_and_lookup_n_alone():
    servers = addresses(11, 40)
    g, o = _gpu_ring(100), OracleRing(100)
    try:
        g.add_remove_servers(servers)
        o.add_remove_servers(servers)
        keys = [f"t-{k}" for k in range(300)]
        g.lookup_ids(keys)
        t = g.last_times()
        assert t[0] > 0 and t[1] > 0
        assert g.last_replica_times() == (0.0, 0.0)
        g.lookup_n_batch(keys, 3)
        tl, tg = g.last_replica_times()
        assert tl > 0 and tg == 0.0
        g.group_replicas(keys, 20)
        assert g.last_replica_times()[1] > 0
        assert g.last_times() == t
        for key, n in (("a random key", 3), ("k2", 20), ("", 39)):
            assert set(g.lookup_n(key, n)) == set(o.lookup_n(key, n))
    finally:
        g.close()
