"""Expected values of the forwarding tests (tests/test_forward_host.py, tests/test_forward.py). TEST INFRASTRUCTURE ONLY.

A numpy restatement of the chain of include/swimsim.h (ABI 16) over the oracle's view-ring owners: owners[h, k] is
owner(h, k) for every row (tests/test_route.py::oracle_owners), live[] and part[] give reach. Nothing here reads the engine.
"""
import numpy as np

LOCAL, DELIVERED, UNREACHABLE, HOP_LIMIT, NO_OWNER, ENTRY_DOWN = range(6)
CHAIN, ONE_HOP = 0, 1
MODES = (0, 1, 2, 3)


def chase(owners, live, part, entry, key, max_hops, policy=CHAIN):
    """(outcome uint8, hops uint8, handler, holder, next int32) of the requests (entry[i], key[i])"""
    owners, live, part = np.asarray(owners, np.int64), np.asarray(live, bool), np.asarray(part, np.int64)
    entry, key = np.asarray(entry, np.int64).reshape(-1), np.asarray(key, np.int64).reshape(-1)
    n = len(entry)
    outcome = np.full(n, ENTRY_DOWN, np.uint8)
    hops = np.zeros(n, np.int64)
    handler, nxt, h = np.full(n, -1, np.int64), np.full(n, -1, np.int64), entry.copy()
    act = np.nonzero(live[entry])[0]                                   # the requests still under way
    for _ in range(max_hops + 1):                                      # every turn ends a chain or adds a hop
        if not len(act):
            break
        d = owners[h[act], key[act]]
        end = np.full(len(act), -1)                                    # the outcome of the chains that end in this turn
        end[d == -1] = NO_OWNER
        here = (end < 0) & (d == h[act])
        end[here] = np.where(hops[act][here] == 0, LOCAL, DELIVERED)
        handler[act[here]] = h[act][here]
        limit = (end < 0) & (hops[act] == max_hops)
        end[limit] = HOP_LIMIT
        dd = np.where(d >= 0, d, 0)
        cut = (end < 0) & ~(live[dd] & (part[dd] == part[h[act]]))
        end[cut] = UNREACHABLE
        nxt[act[limit | cut]] = d[limit | cut]
        go = end < 0
        h[act[go]] = d[go]
        hops[act[go]] += 1
        if policy == ONE_HOP:
            end[go] = DELIVERED
            handler[act[go]] = d[go]
        outcome[act[end >= 0]] = end[end >= 0]
        act = act[end < 0]
    assert not len(act)
    return outcome, hops.astype(np.uint8), handler.astype(np.int32), h.astype(np.int32), nxt.astype(np.int32)


def chase_grid(owners, live, part, entries, max_hops, policy=CHAIN):
    """the five arrays as [len(entries), K]: every key entering at every listed entry (request j * K + k)"""
    K = np.asarray(owners).shape[1]
    e = np.repeat(np.asarray(entries, np.int64), K)
    k = np.tile(np.arange(K), len(entries))
    return tuple(a.reshape(len(entries), K) for a in chase(owners, live, part, e, k, max_hops, policy))


def census(owners, live, part, max_hops, policy=CHAIN):
    """(counted, outcomes[K, 6], hops_hist[K, max_hops + 1], hist_off[K + 1], hist_handler, hist_count): every key entering
    at every live row"""
    entries = np.nonzero(np.asarray(live, bool))[0]
    K = np.asarray(owners).shape[1]
    outcome, hops, handler, _, _ = chase_grid(owners, live, part, entries, max_hops, policy)
    outcomes = np.zeros((K, 6), np.uint32)
    hist = np.zeros((K, max_hops + 1), np.uint32)
    off, mem, cnt = [0], [], []
    for k in range(K):
        if len(entries):
            outcomes[k] = np.bincount(outcome[:, k], minlength=6)
            hist[k] = np.bincount(hops[:, k], minlength=max_hops + 1)
            u, c = np.unique(handler[:, k], return_counts=True)         # ascending: -1 first
            mem += list(u)
            cnt += list(c)
        off.append(len(mem))
    return len(entries), outcomes, hist, np.array(off, np.uint64), np.array(mem, np.int32), np.array(cnt, np.uint32)


def split_keys(want):
    """the keys of a census() result that more than one node handles"""
    off, mem = want[3].astype(np.int64), want[4]
    return int(sum((mem[off[k]:off[k + 1]] >= 0).sum() > 1 for k in range(len(off) - 1)))


def check_census(got, want, what):
    """exact: every bin, every handler entry"""
    assert got[0] == want[0], f"{what}: counted {got[0]}, expected {want[0]}"
    for i, name in ((1, "outcomes"), (2, "hops_hist"), (3, "hist_off"), (4, "hist_handler"), (5, "hist_count")):
        g, w = np.asarray(got[i]), np.asarray(want[i])
        assert g.shape == w.shape and (g == w).all(), f"{what}: {name} differs: engine {g.ravel()[:12]} expected {w.ravel()[:12]}"
    assert (got[1].sum(axis=1) == got[0]).all() and (got[2].sum(axis=1) == got[0]).all()
    assert got[6] >= 0


def check_listed(got, want, what):
    for g, w, name in zip(got[:5], want, ("outcome", "hops", "handler", "holder", "next")):
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {name} is {g.dtype}{g.shape}, expected {w.dtype}{w.shape}"
        bad = np.argwhere(g != w)
        assert not len(bad), f"{what}: {name} of request {tuple(bad[0])}: engine {g[tuple(bad[0])]} expected {w[tuple(bad[0])]} ({len(bad)} differ)"


def check_state(eng, owners, live, part, keys, max_hops=8, policy=CHAIN, R=100, modes=MODES, what=""):
    """the census and the listed call for all entries (dead ones included) in every mode against the restatement;
    returns (listed, census) as expected"""
    n = len(live)
    pol = ("chain", "one_hop")[policy]
    want_l = chase_grid(owners, live, part, np.arange(n), max_hops, policy)
    want_c = census(owners, live, part, max_hops, policy)
    for mode in modes:
        check_listed(eng.forward(keys, np.arange(n), None, max_hops, pol, R, mode), want_l, f"{what} mode {mode} listed")
        check_census(eng.forward_census(keys, max_hops, pol, R, mode), want_c, f"{what} mode {mode} census")
    return want_l, want_c
