"""Checksum-kernel microbench (diagnostic, not the bench): average ms per launch of the checksum kernels over the
first `rows` observer rows of a converged N-member cluster (swimsim_bench_checksum modes: 0 = the production
choice for that many rows, 1 = k_checksum3, 2 = k_checksum_q16, 4 = k_checksum3 with four row groups per
workgroup, 5 = the reference-row path forced). With a 5th argument "verify", rows are perturbed first (one
suspect each) and the checksums of every later mode are compared with the first mode's."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ringpop-go_amd"))
import swimsim  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
rows_list = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [64, 1024, 4096, 16384]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
modes = [int(x) for x in sys.argv[4].split(",")] if len(sys.argv) > 4 else [0, 1, 2]
verify = len(sys.argv) > 5 and sys.argv[5] == "verify"
c = swimsim.Cluster(n, observer_range=(0, min(n, max(rows_list))))
if verify:
    for o in range(min(n, max(rows_list), 4096)):
        c.make_change(o, (o * 7919 + 1) % n, swimsim.T0_MS + 200 * (1 + o % 7), 1)
    c.checksums()
out = {}
for rows in rows_list:
    ref = None
    for mode in modes:
        out[f"rows{rows}_mode{mode}"] = round(c.bench_checksum(rows, mode, reps=reps), 3)
        if verify and mode in (0, 1, 2, 4, 5):
            cs = c.checksums()[:rows].copy()
            if ref is None:
                ref = cs
            else:
                out[f"rows{rows}_mode{mode}_mismatch"] = int((cs != ref).sum())
print(json.dumps(out))
