"""Generates the oracle records of the mass fuzz schedules (tests/fuzz_scenarios.py mass_case, MASS_CASES):

  fuzz_mass_n1100_s0.json, fuzz_mass_n2304_s0.json, fuzz_mass_n4160_s0.json, fuzz_mass_n4160_s1.json

Each file holds, for its case, one record per step call and a final record (tests/fuzz_records.py says what is in
them and how the streams are serialised), under "calls" and "final"; the cases that also run sharded hold the
records of the same case with its direct heals turned into events (fuzz_scenarios.without_direct_heal) under
"sharded", or the word "same" there when the case has no direct heal; and a "reach" block: what the run reached on
the oracle, from rows() snapshots around every round (cells evicted by tombstone timers, the largest evicted member
and evicting observer, the most cells one observer changed in one round), the final counters and the numbers of
events and mutators by kind. tests/test_fuzz_at_size_host.py asserts on that block and regenerates the records on the
single-threaded oracle.

The oracle is oracle/swim_oracle.c built with OpenMP over observers (oracle/build/libswim_oracle_omp.so);
tests/test_oracle_kats.py::test_openmp_oracle_equals_single_thread pins that build to the single-threaded one.
TEST INFRASTRUCTURE ONLY: runs on the CPU; tests/test_fuzz_at_size.py compares the MI355X engine with these files.

usage: python tests/golden/make_fuzz_fixtures.py [N SEED] [threads]     (no case: all of MASS_CASES)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
os.environ["OMP_NUM_THREADS"] = str(min(16, int(sys.argv[3]))) if len(sys.argv) > 3 else "8"
os.environ["ORACLE_LIB"] = os.path.join(REPO, "oracle", "build", "libswim_oracle_omp.so")
sys.path.insert(0, os.path.join(REPO, "tests"))

import fuzz_records as R  # noqa: E402
import fuzz_scenarios as F  # noqa: E402

SHARDED = ((1100, 0), (2304, 0))                                   # the cases tests/test_fuzz_at_size.py also runs sharded


def fixture_name(n, seed):
    return f"fuzz_mass_n{n}_s{seed}.json"


def generate(n, seed):
    c = F.mass_case(n, seed)
    _, out, reach = R.oracle_records(c, reach=True)
    out = dict(n=n, seed=seed, rounds=c["rounds"], reach=reach, **out,
               generator="tests/golden/make_fuzz_fixtures.py (oracle/swim_oracle.c, OpenMP build)")
    if (n, seed) in SHARDED:
        cs = F.without_direct_heal(c)
        out["sharded"] = "same" if cs == c else R.oracle_records(cs)[1]
    with open(os.path.join(HERE, fixture_name(n, seed)), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"{fixture_name(n, seed)}: {reach}", file=sys.stderr, flush=True)


if __name__ == "__main__":
    for n, seed in ([(int(sys.argv[1]), int(sys.argv[2]))] if len(sys.argv) > 2 else F.MASS_CASES):
        generate(n, seed)
