"""Member census and member trace on the device: what they cost.

The state is config 3 (1 % of the members killed in round 10) after round 24, at --members (65,536):
  (a) full      Cluster.census() of every member: device ms (HIP events, the slab pass included) and its rate,
                4 * NL * N bytes / ms, against the 8 TB/s HBM peak; both `who` values.
  (b) list      a census of 64 listed members (k_census_cols): device ms.
  (c) trace     the per-round cost of a 64-member trace: ms_per_step of step(20) over rounds 5-24 with and without the
                trace, --runs fresh clusters each (alternating), every run listed, medians and spread reported. The
                trace's last record is checked against a census of the same members.
  (d) host      at --host-members (4,096): the census (wall time of the whole call) against the host path it replaces,
                Cluster.rows() (one stream round trip per observer) followed by the numpy column counts. The results
                are checked equal. Gate: the census must be at least 10 times faster; the script exits 1 otherwise.
Every timed call runs once untimed first and repeats --reps times; the JSON keeps every repeat and reports the median.
Prints the JSON object and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ringpop-go_amd"))

KILL_ROUND, WARMUP, STEPS = 10, 5, 20
HBM_PEAK_TBS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--host-members", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "census_n65536.json"))
    a = ap.parse_args()

    import numpy as np
    import swimsim
    from swimsim import workloads as W

    med = statistics.median

    def cascade(n, tracked=None):
        """a cluster after rounds 0..24 of config 3, and the ms_per_step of rounds 5-24"""
        wl = W.config3(n=n, rounds=WARMUP + STEPS, kill_round=KILL_ROUND)
        eng = swimsim.Cluster(n, device=0)
        for r in range(WARMUP):
            eng.step(1, wl.events_for(r))
        if tracked is not None:
            eng.trace_members(tracked, 64)
        t0 = time.perf_counter()
        eng.step(STEPS, [e for e in wl.events if e[0] >= WARMUP])
        return eng, (time.perf_counter() - t0) * 1e3 / STEPS

    def timed(f):
        f()
        dev, wall = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = f()
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(r[3])
        return dev, wall

    n = a.members
    killed = [e[2] for e in W.config3(n=n, rounds=WARMUP + STEPS, kill_round=KILL_ROUND).events]
    dead = set(killed)
    alive = [m for m in range(n) if m not in dead]
    tracked = (killed[:32] + alive[:64])[:64]

    # (c) first: the clusters it builds leave the state (a) and (b) measure
    off_ms, on_ms, eng = [], [], None
    for _ in range(a.runs):
        if eng is not None:
            eng.close()
        eng, ms = cascade(n)
        off_ms.append(ms)
        eng.close()
        eng, ms = cascade(n, tracked)
        on_ms.append(ms)
    rounds, nlive, tcounts, dropped = eng.trace()
    assert list(rounds) == list(range(WARMUP, WARMUP + STEPS)) and dropped == 0
    assert (tcounts[-1] == eng.census(tracked)[0]).all() and int(nlive[-1]) == n - len(killed)
    eng.trace_members([])
    trace = {"tracked": len(tracked), "rounds": STEPS, "ms_per_step_without": [round(x, 4) for x in off_ms],
             "ms_per_step_with": [round(x, 4) for x in on_ms], "median_without": round(med(off_ms), 4),
             "median_with": round(med(on_ms), 4), "trace_ms_per_round": round(med(on_ms) - med(off_ms), 4),
             "spread_without": round(max(off_ms) - min(off_ms), 4), "spread_with": round(max(on_ms) - min(on_ms), 4)}

    # (a), (b)
    full = {}
    nbytes = 4.0 * eng.nl * n
    for who in ("live", "all"):
        dev, wall = timed(lambda: eng.census(who=who))
        full[who] = {"device_ms": round(med(dev), 4), "wall_ms": round(med(wall), 3),
                     "tb_per_s": round(nbytes / (med(dev) * 1e-3) / 1e12, 3),
                     "fraction_of_hbm_peak": round(nbytes / (med(dev) * 1e-3) / 1e12 / HBM_PEAK_TBS, 3),
                     "repeats_device_ms": [round(x, 4) for x in dev]}
    dev, wall = timed(lambda: eng.census(tracked))
    lst = {"members": len(tracked), "device_ms": round(med(dev), 4), "wall_ms": round(med(wall), 3),
           "repeats_device_ms": [round(x, 4) for x in dev]}
    counts, _, _, _ = eng.census()
    state = {"round": eng.round, "killed": len(killed), "suspect_cells": int(counts[:, 1].sum()),
             "faulty_cells": int(counts[:, 2].sum())}
    eng.close()

    # (d) the host path at 4,096
    hn = a.host_members
    eng, _ = cascade(hn)
    dev, wall = timed(lambda: eng.census(who="all"))
    got = eng.census(who="all")
    host = []
    for _ in range(max(1, a.reps // 2)):
        t0 = time.perf_counter()
        st, inc = eng.rows()
        st5 = np.where(st == swimsim.UNKNOWN, 5, st)
        hc = np.stack([(st5 == s).sum(axis=0) for s in range(6)], axis=1)
        known = st5 != 5
        hmn = np.where(known, inc, np.iinfo(np.int64).max).min(axis=0)
        hmx = np.where(known, inc, -1).max(axis=0)
        host.append((time.perf_counter() - t0) * 1e3)
    assert (hc == got[0]).all() and (np.where(known.any(axis=0), hmn, -1) == got[1]).all() and (hmx == got[2]).all()
    eng.close()
    ratio = med(host) / med(wall)
    vs_host = {"members": hn, "census_device_ms": round(med(dev), 4), "census_wall_ms": round(med(wall), 3),
               "host_path_wall_ms": round(med(host), 1), "host_over_census": round(ratio, 1),
               "repeats": {"census_wall_ms": [round(x, 3) for x in wall], "host_path_wall_ms": [round(x, 1) for x in host]}}

    ok = ratio >= 10.0
    res = {"members": n, "state": state, "algorithmic_bytes": nbytes, "full": full, "list": lst, "trace": trace,
           "vs_host_path": vs_host, "gate": {"census_at_least_10x_host_path": ok}}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
