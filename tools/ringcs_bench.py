"""Ring checksums through every node's ring view on the device: what they cost.

At --members (65,536), the bench.py cascade (config 3: 1 % of the members killed in round 10), three kinds of state:
  round5    before the kill: every view is the same ring, one chain;
  wave      after each of --wave-rounds (inside the faulty wave: node by node the suspects turn faulty, many views);
  round99   after the last round: the live nodes agree again, the killed nodes' rows keep their own views.
For each state, after one untimed call, --runs times:
  census    Cluster.ring_census("live"): the device ms of the `ms` out-parameter and its split over the scan, the exact
            comparison ("group") and the chains with their scatter ("hash") from Cluster.ring_times(); the chains run
            (`hashed`), the distinct checksums, the host wall time of the call;
  rows      Cluster.ring_checksums() of every row (who = all, with the read-back of 8 bytes per row);
  one_chain Cluster.ring_checksums([o], mode 1) of one live observer: one workgroup, one chain; ns per 20-byte block.
Comparison with the only way there was before these calls, at --small (4,096) members in the same cascade, inside the
wave: one Cluster.row() read-back per observer and the host hashing the joined addresses (the oracle's C Fingerprint32,
once per distinct presence set), against Cluster.ring_checksums() of every row; both wall times, and the two results
must be equal. The tool fails when the new call is slower than that method.
Prints the JSON object and writes it to --out; medians and the spread (max - min) of the runs are reported, every run is
kept.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ringpop-go_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))                       # oracle_ffi: the host Fingerprint32 of the comparison

KILL_ROUND = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--small", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--wave-rounds", type=int, nargs="+", default=[36, 38, 40, 42])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ringcs_n65536.json"))
    a = ap.parse_args()

    import numpy as np
    import swimsim
    from swimsim import metrics
    from swimsim import workloads as W

    med = statistics.median

    def stats(xs):
        return {"median_ms": round(med(xs), 4), "spread_ms": round(max(xs) - min(xs), 4), "runs_ms": [round(x, 4) for x in xs]}

    def timed(f):
        """[(result, wall ms, (scan, group, hash) ms)] of --runs calls after one untimed call"""
        f()
        out = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            r = f()
            out.append((r, (time.perf_counter() - t0) * 1e3, eng.ring_times()))
        return out

    def measure(label):
        width = len(eng.address(0))
        runs = timed(lambda: eng.ring_census("live"))
        counted, cs, cnt, srv, first, hashed, _ = runs[0][0]
        ag = metrics.ring_agreement(counted, cs, cnt)
        rec = {"round": eng.round - 1, "counted_rows": counted, "distinct_checksums": ag.distinct,
               "majority_share": round(ag.share, 6), "hashed": hashed,
               "census": stats([r[0][6] for r in runs]), "census_wall_ms": round(med([r[1] for r in runs]), 3),
               "scan": stats([r[2][0] for r in runs]), "group": stats([r[2][1] for r in runs]),
               "hash": stats([r[2][2] for r in runs]),
               "scan_row_tb_per_s": round(4.0 * npad * counted / (med([r[2][0] for r in runs]) * 1e-3) / 1e12, 3)}
        runs = timed(lambda: eng.ring_checksums())
        rec["rows_all"] = {"rows": n, "hashed": runs[0][0][2], "device": stats([r[0][3] for r in runs]),
                           "wall_ms": round(med([r[1] for r in runs]), 3)}
        o = int(first[int(np.argmax(cnt))])                            # an observer of the majority view
        runs = timed(lambda: eng.ring_checksums([o], 1))
        servers = int(runs[0][0][1][0])
        blocks = max(1, (servers * (width + 1) - 2) // 20)
        hash_ms = med([r[2][2] for r in runs])
        rec["one_chain"] = {"observer": o, "servers": servers, "blocks": blocks, "hash": stats([r[2][2] for r in runs]),
                            "scan": stats([r[2][0] for r in runs]), "ns_per_block": round(hash_ms * 1e6 / blocks, 2)}
        print(label, json.dumps(rec), flush=True)
        return rec

    def step_to(upto):
        while eng.round < upto:
            eng.step(1, wl.events_for(eng.round))

    n = a.members
    npad = (n + 63) // 64 * 64
    wl = W.config3(n=n, rounds=a.rounds, kill_round=KILL_ROUND)
    res = {"members": n, "workload": wl.name, "chunk": swimsim.RING_CHECKSUM_CHUNK, "states": {}}
    eng = swimsim.Cluster(n, device=0)
    try:
        mem0 = eng.memory()["total"]
        step_to(6)
        res["states"]["round5"] = measure("round5")
        res["scratch_bytes"] = eng.memory()["total"] - mem0
        res["states"]["wave"] = []
        for r in a.wave_rounds:
            step_to(r + 1)
            res["states"]["wave"].append(measure(f"wave round {r}"))
        step_to(a.rounds)
        res["states"][f"round{a.rounds - 1}"] = measure(f"round{a.rounds - 1}")
    finally:
        eng.close()

    # the comparison: one row read-back per observer and host hashing, against the new call, inside the wave
    from oracle_ffi import fingerprint32
    n = a.small
    wl = W.config3(n=n, rounds=50, kill_round=KILL_ROUND)
    eng = swimsim.Cluster(n, device=0)
    try:
        step_to(39)
        addr = [eng.address(m) for m in range(n)]

        def by_rows():
            out = np.empty(n, np.uint32)
            views = {}
            for o in range(n):
                present = eng.row(o)[0] <= 1
                key = present.tobytes()
                if key not in views:
                    views[key] = fingerprint32(";".join(addr[m] for m in np.nonzero(present)[0]).encode())
                out[o] = views[key]
            return out, len(views)

        old_wall, new_wall = [], []
        want, views = by_rows()
        eng.ring_checksums()
        for _ in range(a.runs):                                        # alternating, in the same process
            t0 = time.perf_counter()
            want, views = by_rows()
            old_wall.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            got, _, hashed, dev_ms = eng.ring_checksums()
            new_wall.append((time.perf_counter() - t0) * 1e3)
        equal = bool((got == want).all())
        res["comparison"] = {"members": n, "round": eng.round - 1, "distinct_views": views, "hashed": hashed,
                             "row_readbacks_and_host_hash_wall": stats(old_wall), "ring_checksums_wall": stats(new_wall),
                             "ring_checksums_device_ms": round(dev_ms, 4), "results_equal": equal,
                             "speedup": round(med(old_wall) / med(new_wall), 1),
                             "not_slower": bool(med(new_wall) <= med(old_wall))}
        print("comparison", json.dumps(res["comparison"]), flush=True)
    finally:
        eng.close()

    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    ok = res["comparison"]["results_equal"] and res["comparison"]["not_slower"]
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
