"""Requests forwarded through every node's ring view on the device: what it costs.

State: --members (65,536), config 3 with 1 % of the members killed in round 3, stepped through round 30: the live nodes
drop the killed members one by one there, so the views disagree, requests die at the entry node and one hop in.
Keys: "key-0" .. "key-(K-1)", K = --keys (1,024: one pass of the owner table at 65,536 rows); max_hops 8, policy chain.
Timed, alternating in one process after one untimed call of each, --runs times (at least 5):
  forward_census   Cluster.forward_census(keys): the device ms of the `ms` out-parameter, with the split of
                   Cluster.forward_times() over the owner table, the chases and the rest (key hashes, pair sort, run count);
  route_census     Cluster.route_census(keys, "live") on the same state and keys: the yardstick. Its code is the parent
                   commit's, and forward_census performs the same rows x keys lookups before it follows the chains.
Reported: the medians and spreads, every run, the ratio of the medians, the headline of the census (served share, split
keys, outcome and hop totals), the owner table's bytes and the rate at which it is written and gathered, and the same
census in the converged state before the kill (no forward fails). The listed call is timed for 64 entries x K keys.
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

KILL_ROUND = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--keys", type=int, default=1024)
    ap.add_argument("--round", type=int, default=30, help="the state after this round")
    ap.add_argument("--max-hops", type=int, default=8)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "forward_n65536.json"))
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: at least 5 timed calls")

    import numpy as np
    import swimsim
    from swimsim import metrics
    from swimsim import workloads as W

    med = statistics.median

    def stats(xs):
        return {"median_ms": round(med(xs), 4), "spread_ms": round(max(xs) - min(xs), 4), "runs_ms": [round(x, 4) for x in xs]}

    n, K = a.members, a.keys
    keys = [f"key-{i}" for i in range(K)]
    wl = W.config3(n=n, rounds=a.round + 10, kill_round=KILL_ROUND)
    eng = swimsim.Cluster(n, device=0)

    def measure(label):
        eng.forward_census(keys, a.max_hops)                          # untimed: first-use allocations, code objects
        eng.route_census(keys, "live")
        fwd, route, split, wall = [], [], [], []
        for _ in range(a.runs):                                        # alternating: both see the same machine
            t0 = time.perf_counter()
            r = eng.forward_census(keys, a.max_hops)
            wall.append((time.perf_counter() - t0) * 1e3)
            fwd.append(r[6])
            split.append(eng.forward_times())
            route.append(eng.route_census(keys, "live")[4])
        counted = r[0]
        av = metrics.forward_availability(*r[:6])
        table, chase, hist = (med([s[i] for s in split]) for i in range(3))
        table_bytes = 4 * counted * K                                 # one 4-byte cell per live row and key
        out = {
            "forward_census": stats(fwd), "forward_census_wall_ms": round(med(wall), 3), "route_census": stats(route),
            "forward_over_route": round(med(fwd) / med(route), 3),
            "split_ms": {"table": round(table, 4), "chase": round(chase, 4), "hist": round(hist, 4)},
            "counted_entries": counted, "requests": av.requests, "requests_per_s": round(av.requests / (med(fwd) * 1e-3), 1),
            "owner_table_bytes": table_bytes,
            "table_write_gb_per_s": round(table_bytes / (table * 1e-3) / 1e9, 2),
            "chase_gathers_per_s": round(float((av.hops_total * (np.arange(a.max_hops + 1) + 1)).sum()) / (chase * 1e-3), 1),
            "served_share": round(av.served_total / av.requests, 6), "split_keys": av.split_keys,
            "outcome_totals": dict(zip(swimsim.FWD_OUTCOMES, (int(x) for x in av.outcome_totals))),
            "hops_totals": [int(x) for x in av.hops_total], "handler_entries": int(len(r[4]))}
        print(label, json.dumps(out), flush=True)
        return out

    res = {"members": n, "keys": K, "replica_points": 100, "max_hops": a.max_hops, "policy": "chain", "kill_round": KILL_ROUND,
           "killed": len(wl.events), "states": {}}
    try:
        eng.step(KILL_ROUND, [e for e in wl.events if e[0] < KILL_ROUND])
        res["states"]["converged"] = measure("converged")
        while eng.round <= a.round:
            eng.step(1, wl.events_for(eng.round))
        res["states"][f"round{a.round}"] = measure(f"round{a.round}")
        # the listed call: 64 entries x K keys
        ent = list(range(0, n, max(1, n // 64)))[:64]
        eng.forward(keys, ent, None, a.max_hops)
        listed, lsplit = [], []
        for _ in range(a.runs):
            listed.append(eng.forward(keys, ent, None, a.max_hops)[5])
            lsplit.append(eng.forward_times())
        res["forward_64_entries"] = dict(stats(listed), table_ms=round(med([s[0] for s in lsplit]), 4),
                                         chase_ms=round(med([s[1] for s in lsplit]), 4))
        res["memory_total_bytes"] = eng.memory()["total"]
    finally:
        eng.close()
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
