"""Scenarios of the option tests (tests/test_options_host.py on the CPU oracle, tests/test_options.py engine against
oracle). TEST INFRASTRUCTURE ONLY.

Four fields of swimsim_config change what the round kernels do: ping_request_size (K), max_reverse_full_sync_jobs,
p_factor and seed. Each scenario below is built to reach the code one of them steers:

  P  a partition that cuts five members off for twelve rounds: failed pings whose helpers partly fail too, so the
     ping-req phases run with every mix of helper answers and helper errors (K indexes all of their buffers);
  T  six members, two dead, one cut off: fewer eligible helpers than K, all of them failing (node.go:497: the run
     is inconclusive only at len(errs) == PingRequestSize);
  S  200 nodes that know themselves and members 0..3 only: rows with about 4 pingable members out of 200, so the 64
     helper draws run dry and the helper search walks the row; full syncs and reverse full syncs fill the job queues;
  M  one long-lived rumour under a large pFactor: the piggyback count climbs to maxP - 1, the top of what the
     engine's 8-bit counter may hold.
"""
from oracle_ffi import OracleSim, philox
from swimsim import workloads as W

T0_MS = 1_500_000_000_000
ALIVE = 0

# ---- P: partition (for K) -------------------------------------------------------------------------------------------
P_N, P_ROUNDS = 70, 45                                # NP = 128: two bitmap words
P_CUT = (3, 17, 40, 64, 69)
P_EVENTS = ([(0, W.EV_KILL, 5, 0), (0, W.EV_KILL, 33, 0)] +
            [(2, W.EV_PARTITION, m, 1) for m in P_CUT] + [(14, W.EV_PARTITION, m, 0) for m in P_CUT] +
            [(20, W.EV_REVIVE, 5, 0), (22, W.EV_LEAVE, 9, 0)])
P_KS = (1, 2, 5, 8)

# ---- T: tiny (eligible < K) -----------------------------------------------------------------------------------------
T_N, T_ROUNDS = 6, 40
T_EVENTS = [(0, W.EV_KILL, 1, 0), (0, W.EV_KILL, 2, 0), (3, W.EV_PARTITION, 3, 1), (9, W.EV_PARTITION, 3, 0)]

# ---- S: sparse rows -------------------------------------------------------------------------------------------------
S_N, S_ROUNDS = 200, 14
S_SEEDS = (0, 1, 2, 3)
S_EVENTS = [(0, W.EV_KILL, 3, 0)]

# ---- M: long-lived rumour (n, p_factor, rounds); maxP = p_factor * digits10(pingable) ---------------------------------
M_EVENTS = [(0, W.EV_KILL, 5, 0)]
M_CASES = ((12, 127, 300), (130, 85, 200), (102, 85, 200))


def digits10(n):
    d = 0
    while n > 0:
        d, n = d + 1, n // 10
    return d


def m_maxp(n, p_factor):
    """maxP of scenario M's rows: one member dead, every other one pingable"""
    return p_factor * digits10(n - 2)


def run_oracle(n, rounds, events, each_round=None, **kw):
    ora = OracleSim(n, **kw)
    for r in range(rounds):
        ora.step([e for e in events if e[0] == r])
        if each_round:
            each_round(ora, r)
    return ora


def seed_sparse(sims, n=S_N):
    """scenario S's start on every simulator of `sims` (created with init="self"): each node learns members 0..3 by
    MakeChange. Returns the calls' results per simulator, which must be equal."""
    out = [[] for _ in sims]
    for o in range(n):
        for m in S_SEEDS:
            if m != o:
                for i, s in enumerate(sims):
                    out[i].append(s.make_change(o, m, T0_MS, ALIVE))
    return out


def sparse_oracle(**kw):
    ora = OracleSim(S_N, init="self", **kw)
    seed_sparse([ora])
    return ora


def largest_p(ora):
    return max((e[0] for o in range(ora.n) for e in ora.dis_entries(o).values()), default=-1)


def walk_events(ora_kw, n=S_N, rounds=S_ROUNDS, events=S_EVENTS, per_round=None):
    """Runs scenario S on the oracle and counts the failed pings whose helper search needs the walk: the 64 Philox
    draws of RandomPingableMembers (docs/ROUND_SEMANTICS.md §3: draw i is word i & 3 of the block at counter
    (round, observer, 2, i >> 2), scaled to [0, n) by the high half of the product) find fewer than
    min(K, eligible) distinct eligible members. The draws are taken against the oracle's rows before the round; the
    oracle draws after the round's direct pings have merged, when a row may hold a few more members, so this is an
    estimate (a guard takes a wide margin), not the oracle's own count. Returns (events, the oracle after the run)."""
    seed = ora_kw.get("seed", 1)
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    K = ora_kw.get("ping_request_size", 3)
    ora = sparse_oracle(**ora_kw)
    live, part = [True] * n, [0] * n
    walks = 0
    for r in range(rounds):
        evr = [e for e in events if e[0] == r]
        for (_, kind, a, b) in evr:
            if kind in (W.EV_KILL, W.EV_REVIVE):
                live[a] = kind == W.EV_REVIVE
            elif kind == W.EV_PARTITION:
                part[a] = b
        st, _ = ora.rows()
        ora.step(evr)
        tg = ora.last_targets()
        here = 0
        for o in range(n):
            t = int(tg[o])
            if t < 0 or not live[o] or (live[t] and part[t] == part[o]):
                continue                                              # no ping, or the ping arrived
            ok = [m != o and m != t and int(st[o][m]) <= 1 for m in range(n)]   # pingable: alive or suspect
            need = min(K, sum(ok))
            got, blk = set(), None
            for i in range(64):
                if len(got) >= need:
                    break
                if i & 3 == 0:
                    blk = philox([r, o, 2, i >> 2], key)
                c = (blk[i & 3] * n) >> 32
                if ok[c]:
                    got.add(c)
            here += int(len(got) < need)
        if per_round is not None:
            per_round.append(here)
        walks += here
    return walks, ora
