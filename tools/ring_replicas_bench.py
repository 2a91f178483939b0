"""LookupN on the device ring: one call per key against one batched call, and the replica grouping.

The ring is that of a converged cluster: --members servers (swimsim.address_of), --replicas points each. Three
measurements, all at n = --n (the replicator's default NValue is 3):
  (a) per_key    --loop-keys calls of HashRing.lookup_n(key, n): one launch and two synchronisations per key,
                 the only way to ask for LookupN before the batched entry point. Wall time per key.
  (b) batched    one HashRing.lookup_n_ids call of --keys keys: kernel ms (swimring_last_replica_times) and wall
                 time (the whole Python call, key packing included; c_call_wall_ms is the C call alone), both
                 also per key, beside lookup_ids on the same keys (swimring_last_times): Lookup is the n = 1
                 floor, it pays the same hash and binary search.
  (c) grouped    the same batch through group_replica_ids: kernel ms of the lookup and of the grouping
                 (sort + boundaries), wall time.
Every timed shape runs once untimed first; timed calls repeat --reps times and the JSON keeps every repeat and
reports the median. Gate: the batched wall time per key must be below (a)'s; the script exits 1 otherwise.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=8192)
    ap.add_argument("--replicas", type=int, default=100)
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--loop-keys", type=int, default=4096)
    ap.add_argument("--n", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ring_replicas_bench.json"))
    a = ap.parse_args()

    import numpy as np
    from swimsim import address_of
    from swimsim.ring import HashRing, _lib, _pack

    ring = HashRing(a.replicas, device=0)
    ring.add_remove_servers([address_of(m) for m in range(a.members)])
    points = len(ring.points()[0])
    keys = [f"key-{k}" for k in range(a.keys)]
    med = statistics.median

    # (a) one call per key
    for k in keys[:64]:
        ring.lookup_n(k, a.n)
    t0 = time.perf_counter()
    for k in keys[:a.loop_keys]:
        ring.lookup_n(k, a.n)
    loop_s = time.perf_counter() - t0
    per_key = {"calls": a.loop_keys, "wall_ms": round(loop_s * 1e3, 3), "wall_us_per_key": round(loop_s * 1e6 / a.loop_keys, 3)}

    # (b) one batched call, and Lookup on the same keys
    ring.lookup_n_ids(keys, a.n)
    ring.lookup_ids(keys)
    blob, off = _pack(keys)
    out = np.empty((a.keys, a.n), np.int32)
    cnt = np.empty(a.keys, np.uint32)
    kern, wall, cwall, look, look_wall = [], [], [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ids, _ = ring.lookup_n_ids(keys, a.n)
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(ring.last_replica_times()[0])
        t0 = time.perf_counter()
        rc = _lib().swimring_lookup_n_batch(ring.h, blob, off.ctypes.data, a.keys, a.n, out.ctypes.data, cnt.ctypes.data)
        cwall.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0 and (out == ids).all()
        t0 = time.perf_counter()
        first = ring.lookup_ids(keys)
        look_wall.append((time.perf_counter() - t0) * 1e3)
        look.append(ring.last_times()[1])
        assert (first == ids[:, 0]).all()
    batched = {
        "keys": a.keys, "kernel_ms": round(med(kern), 4), "kernel_ns_per_key": round(med(kern) * 1e6 / a.keys, 3),
        "wall_ms": round(med(wall), 3), "wall_us_per_key": round(med(wall) * 1e3 / a.keys, 4),
        "c_call_wall_ms": round(med(cwall), 3), "c_call_wall_us_per_key": round(med(cwall) * 1e3 / a.keys, 4),
        "lookup_kernel_ms": round(med(look), 4), "lookup_kernel_ns_per_key": round(med(look) * 1e6 / a.keys, 3),
        "lookup_wall_ms": round(med(look_wall), 3),
        "kernel_per_key_vs_lookup": round(med(kern) / med(look), 3) if med(look) > 0 else None,
        "repeats": {"kernel_ms": [round(x, 4) for x in kern], "wall_ms": [round(x, 3) for x in wall],
                    "c_call_wall_ms": [round(x, 3) for x in cwall], "lookup_kernel_ms": [round(x, 4) for x in look]},
    }

    # (c) the same batch through groupReplicas
    ring.group_replica_ids(keys, a.n)
    gk, gg, gw = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        gids, gcnt, dest, doff, kidx = ring.group_replica_ids(keys, a.n)
        gw.append((time.perf_counter() - t0) * 1e3)
        lk, gr = ring.last_replica_times()
        gk.append(lk)
        gg.append(gr)
        assert (gids == ids).all() and int(doff[-1]) == int(gcnt.sum()) == len(kidx)
    grouped = {
        "keys": a.keys, "entries": int(doff[-1]), "destinations": len(dest), "lookup_n_kernel_ms": round(med(gk), 4),
        "group_ms": round(med(gg), 4), "group_ns_per_key": round(med(gg) * 1e6 / a.keys, 3), "wall_ms": round(med(gw), 3),
        "repeats": {"group_ms": [round(x, 4) for x in gg], "wall_ms": [round(x, 3) for x in gw]},
    }
    ring.close()

    ok = batched["wall_us_per_key"] < per_key["wall_us_per_key"]
    res = {"servers": a.members, "replica_points": a.replicas, "points": points, "n": a.n, "per_key": per_key,
           "batched": batched, "grouped": grouped,
           "gate": {"batched_wall_below_per_key_wall": ok,
                    "per_key_over_batched_wall": round(per_key["wall_us_per_key"] / batched["wall_us_per_key"], 1)}}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
