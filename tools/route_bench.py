"""Key routing through every node's ring view on the device: what it costs.

States, at --members (65,536), config 3 (1 % of the members killed in round 10):
  converged   the fresh cluster: every view is the same ring;
  round24     after round 24: the killed members are suspect in most rows, and suspects are still servers;
  wave        after each of rounds 35 to 44, the faulty wave: node by node the suspects turn faulty and the live nodes
              disagree on the keys the killed members owned (the census's exception pairs, their sort and run-length
              encoding are at work). Only the census of 4,096 keys is timed there, with its exception pairs.
For each state and K = 256 and 4,096 keys ("key-i"), --runs times each after one untimed call:
  census      Cluster.route_census(keys, "live"): the device ms of the `ms` out-parameter (key hashing, the base row, the
              pass over the rows, sort and run-length encoding), lookups/s (counted rows x K / ms) and row bytes/s
              (4 * NP * counted rows / ms);
  route       Cluster.route of 64 observers: device ms.
Yardstick: the full member census of the same state in the same session (Cluster.census(), the same row stream); the
ratio route census / member census is recorded per state and K.
Direct path: a self-only start (every node knows itself and two seed members) at --self-members after 1 and after 3
rounds: the census in mode 0 (the direct path for the rows whose cnt servers satisfy cnt * cnt * R <= N, the walk for
the others), and Cluster.route of 8 observers in mode 2 (direct) against mode 1 (the ring walk, which meets a server
only every N / cnt points).
Prints the JSON object and writes it to --out; medians and the spread (max - min) of the runs are reported, every run
is kept.

--n N [N ...] measures the replica-set calls instead and leaves the above alone: for the same states
and key counts, Cluster.replica_census(keys, n, "live") beside Cluster.route_census(keys, "live") and the member census
of the same state in the same session, with the ratios; across the faulty wave the census of 4,096 keys with its
exception pairs (counted from the result: per key, the rows that miss a member of the first counted row's set plus the
rows that list a member outside it); and at the self-only start Cluster.route_n of 8 observers, walk against direct.
The default --out is then profiles/route_n_n65536.json.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ringpop-go_amd"))

KILL_ROUND = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--self-members", type=int, default=16384)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, nargs="+", default=None, help="replica-set sizes: measure route_n / replica_census")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(REPO, "profiles", "route_n_n65536.json" if a.n else "route_n65536.json")

    import numpy as np
    import swimsim
    from swimsim import metrics
    from swimsim import workloads as W

    med = statistics.median

    def stats(xs):
        return {"median_ms": round(med(xs), 4), "spread_ms": round(max(xs) - min(xs), 4), "runs_ms": [round(x, 4) for x in xs]}

    def timed(f, ms_of):
        f()
        dev, wall = [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            r = f()
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(ms_of(r))
        return dev, wall

    def measure(eng, n, label):
        npad = (n + 63) // 64 * 64
        dev, _ = timed(lambda: eng.census(), lambda r: r[3])
        out = {"member_census": stats(dev), "keys": {}}
        yard = med(dev)
        for K in (256, 4096):
            keys = [f"key-{i}" for i in range(K)]
            dev, wall = timed(lambda: eng.route_census(keys, "live"), lambda r: r[4])
            counted, off, own, cnt, _ = eng.route_census(keys, "live")
            ag = metrics.route_agreement(counted, off, own, cnt)
            m = med(dev)
            obs = list(range(0, n, max(1, n // 64)))[:64]
            rdev, _ = timed(lambda: eng.route(keys, obs), lambda r: eng.last_route_ms)
            out["keys"][str(K)] = {
                "census": stats(dev), "census_wall_ms": round(med(wall), 3), "counted_rows": counted,
                "lookups_per_s": round(counted * K / (m * 1e-3), 1),
                "row_tb_per_s": round(4.0 * npad * counted / (m * 1e-3) / 1e12, 3),
                "over_member_census": round(m / yard, 3),
                "keys_disagreed": int((ag.distinct > 1).sum()), "histogram_entries": int(len(own)),
                "exception_pairs": int(counted * K - ag_base(counted, off, own, cnt, eng, keys)),
                "route_64_observers": stats(rdev)}
        print(label, json.dumps(out), flush=True)
        return out

    def ag_base(counted, off, own, cnt, eng, keys):
        """rows that answer the first counted row's owner, summed over the keys (the pairs the device does not append)"""
        first = next(o for o in range(eng.n) if eng_live[o])
        base = eng.route(keys, [first])[0]
        tot = 0
        for k in range(len(keys)):
            sl = slice(int(off[k]), int(off[k + 1]))
            hit = np.nonzero(own[sl] == base[k])[0]
            tot += int(cnt[sl][hit[0]]) if len(hit) else 0
        return tot

    def finish(res):
        print(json.dumps(res, indent=1))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return 0

    if a.n:
        return finish(replica_sets(a, stats, timed))

    n = a.members
    wl = W.config3(n=n, rounds=50, kill_round=KILL_ROUND)
    eng_live = np.ones(n, bool)
    res = {"members": n, "replica_points": 100, "states": {}}
    eng = swimsim.Cluster(n, device=0)
    try:
        t0 = time.perf_counter()
        eng.route_census(["warm"], "live")
        res["point_table_first_use_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        res["states"]["converged"] = measure(eng, n, "converged")
        def step_to(upto):
            while eng.round < upto:
                ev = wl.events_for(eng.round)
                for e in ev:
                    if e[1] == W.EV_KILL:
                        eng_live[e[2]] = False
                eng.step(1, ev)

        step_to(25)
        res["states"]["round24"] = measure(eng, n, "round24")
        keys = [f"key-{i}" for i in range(4096)]
        res["faulty_wave"] = []
        for r in range(35, 45):
            step_to(r + 1)
            dev, _ = timed(lambda: eng.route_census(keys, "live"), lambda x: x[4])
            counted, off, own, cnt, _ = eng.route_census(keys, "live")
            ag = metrics.route_agreement(counted, off, own, cnt)
            rec = {"round": r, "keys": 4096, "census": stats(dev), "counted_rows": counted,
                   "keys_disagreed": int((ag.distinct > 1).sum()), "histogram_entries": int(len(own)),
                   "exception_pairs": int(counted * 4096 - ag_base(counted, off, own, cnt, eng, keys))}
            print("wave", json.dumps(rec), flush=True)
            res["faulty_wave"].append(rec)
        res["memory_total_bytes"] = eng.memory()["total"]
    finally:
        eng.close()

    # the direct path: a self-only start
    sn = a.self_members
    eng_live = np.ones(sn, bool)
    eng = swimsim.Cluster(sn, device=0, init="self")
    try:
        for o in range(sn):
            for m in (0, 1):
                if m != o:
                    eng.make_change(o, m, swimsim.T0_MS, swimsim.ALIVE)
        keys = [f"key-{i}" for i in range(256)]
        obs = list(range(0, sn, sn // 8))[:8]
        res["self_only_start"] = []
        for upto in (1, 3):
            eng.step(upto - eng.round)
            counts = eng.census()[0]
            dev, _ = timed(lambda: eng.route_census(keys, "live", 100, 0), lambda r: r[4])
            d2, _ = timed(lambda: eng.route(keys, obs, 100, 2), lambda r: eng.last_route_ms)
            d1, _ = timed(lambda: eng.route(keys, obs, 100, 1), lambda r: eng.last_route_ms)
            assert (eng.route(keys, obs, 100, 1) == eng.route(keys, obs, 100, 2)).all()
            rec = {"members": sn, "rounds_run": eng.round, "keys": 256,
                   "servers_per_row_mean": round(float(counts[:, :2].sum()) / sn, 2),
                   "direct_in_mode0_up_to_servers": int((sn / 100) ** 0.5),
                   "census_mode0": stats(dev), "lookups_per_s": round(sn * 256 / (med(dev) * 1e-3), 1),
                   "route_8_observers_direct": stats(d2), "route_8_observers_walk": stats(d1)}
            print("self", json.dumps(rec), flush=True)
            res["self_only_start"].append(rec)
    finally:
        eng.close()

    return finish(res)


def replica_sets(a, stats, timed):
    """the --n measurement: replica_census against route_census and the member census, state by state"""
    import numpy as np
    import swimsim
    from swimsim import metrics
    from swimsim import workloads as W

    med = statistics.median

    def pairs(eng, keys, nn, first, counted, off, mem, cnt):
        """exception pairs the device appended: rows that miss a base member + rows that list a member outside the base"""
        base = eng.route_n(keys, [first], nn)[0][0]
        key = np.repeat(np.arange(len(keys)), np.diff(off).astype(np.int64))
        inbase = (base[key] == mem[:, None]).any(axis=1)
        return int((counted - cnt[inbase].astype(np.int64)).sum() + cnt[~inbase].astype(np.int64).sum())

    def measure(eng, n, first, label):
        dev, _ = timed(lambda: eng.census(), lambda r: r[3])
        out = {"member_census": stats(dev), "keys": {}}
        yard = med(dev)
        for K in (256, 4096):
            keys = [f"key-{i}" for i in range(K)]
            rdev, _ = timed(lambda: eng.route_census(keys, "live"), lambda r: r[4])
            rec = {"route_census": stats(rdev), "route_census_over_member_census": round(med(rdev) / yard, 3), "n": {}}
            for nn in a.n:
                dev, wall = timed(lambda: eng.replica_census(keys, nn, "live"), lambda r: r[4])
                counted, off, mem, cnt, _ = eng.replica_census(keys, nn, "live")
                ag = metrics.replica_agreement(counted, off, mem, cnt, nn)
                rec["n"][str(nn)] = {
                    "replica_census": stats(dev), "wall_ms": round(med(wall), 3), "counted_rows": counted,
                    "over_route_census": round(med(dev) / med(rdev), 3), "over_member_census": round(med(dev) / yard, 3),
                    "keys_disagreed": int((~ag.agreed).sum()), "histogram_entries": int(len(mem)),
                    "exception_pairs": pairs(eng, keys, nn, first, counted, off, mem, cnt)}
            out["keys"][str(K)] = rec
        print(label, json.dumps(out), flush=True)
        return out

    n = a.members
    wl = W.config3(n=n, rounds=50, kill_round=KILL_ROUND)
    live = np.ones(n, bool)
    res = {"members": n, "replica_points": 100, "n": a.n, "states": {}}
    eng = swimsim.Cluster(n, device=0)
    try:
        eng.route_census(["warm"], "live")

        def step_to(upto):
            while eng.round < upto:
                ev = wl.events_for(eng.round)
                for e in ev:
                    if e[1] == W.EV_KILL:
                        live[e[2]] = False
                eng.step(1, ev)

        first = lambda: int(np.nonzero(live)[0][0])
        res["states"]["converged"] = measure(eng, n, first(), "converged")
        step_to(25)
        res["states"]["round24"] = measure(eng, n, first(), "round24")
        step_to(42)
        res["states"]["round41"] = measure(eng, n, first(), "round41")
        res["memory_total_bytes_after_round41"] = eng.memory()["total"]
    finally:
        eng.close()
    # the faulty wave, round by round (a fresh cluster: the states above are measured at rounds inside it)
    live[:] = True
    eng = swimsim.Cluster(n, device=0)
    try:
        keys = [f"key-{i}" for i in range(4096)]
        res["faulty_wave"] = []
        for r in range(35, 45):
            while eng.round < r + 1:
                ev = wl.events_for(eng.round)
                for e in ev:
                    if e[1] == W.EV_KILL:
                        live[e[2]] = False
                eng.step(1, ev)
            f0 = int(np.nonzero(live)[0][0])
            rdev, _ = timed(lambda: eng.route_census(keys, "live"), lambda x: x[4])
            rec = {"round": r, "keys": 4096, "route_census": stats(rdev), "n": {}}
            for nn in a.n:
                dev, _ = timed(lambda: eng.replica_census(keys, nn, "live"), lambda x: x[4])
                counted, off, mem, cnt, _ = eng.replica_census(keys, nn, "live")
                ag = metrics.replica_agreement(counted, off, mem, cnt, nn)
                rec["n"][str(nn)] = {"replica_census": stats(dev), "counted_rows": counted,
                                     "over_route_census": round(med(dev) / med(rdev), 3),
                                     "keys_disagreed": int((~ag.agreed).sum()), "histogram_entries": int(len(mem)),
                                     "exception_pairs": pairs(eng, keys, nn, f0, counted, off, mem, cnt)}
            print("wave", json.dumps(rec), flush=True)
            res["faulty_wave"].append(rec)
    finally:
        eng.close()
    # the direct path: a self-only start
    sn = a.self_members
    eng = swimsim.Cluster(sn, device=0, init="self")
    try:
        for o in range(sn):
            for m in (0, 1):
                if m != o:
                    eng.make_change(o, m, swimsim.T0_MS, swimsim.ALIVE)
        keys = [f"key-{i}" for i in range(256)]
        obs = list(range(0, sn, sn // 8))[:8]
        res["self_only_start"] = []
        for upto in (1, 3):
            eng.step(upto - eng.round)
            counts = eng.census()[0]
            rec = {"members": sn, "rounds_run": eng.round, "keys": 256,
                   "servers_per_row_mean": round(float(counts[:, :2].sum()) / sn, 2),
                   "servers_of_the_8_observers": [int(x) for x in eng.route_n(keys, obs, 1)[1]],
                   "direct_in_mode0_up_to_servers": int((sn / 100) ** 0.5), "n": {}}
            for nn in a.n:
                d2, _ = timed(lambda: eng.route_n(keys, obs, nn, 100, 2), lambda r: eng.last_route_ms)
                d1, _ = timed(lambda: eng.route_n(keys, obs, nn, 100, 1), lambda r: eng.last_route_ms)
                dev, _ = timed(lambda: eng.replica_census(keys, nn, "live", 100, 0), lambda r: r[4])
                assert (eng.route_n(keys, obs, nn, 100, 1)[0] == eng.route_n(keys, obs, nn, 100, 2)[0]).all()
                rec["n"][str(nn)] = {"route_n_8_observers_direct": stats(d2), "route_n_8_observers_walk": stats(d1),
                                     "census_mode0": stats(dev)}
            print("self", json.dumps(rec), flush=True)
            res["self_only_start"].append(rec)
    finally:
        eng.close()
    return res


if __name__ == "__main__":
    sys.exit(main())
