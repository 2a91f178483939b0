"""bench.py's launch contract on CPU (no GPU call): `--gpus N` without a launcher starts N ranks itself
through a child torch.distributed.run, and the workload accounting counts live members only. One GPU test: a plain
run's line and its --dump-outputs arrays."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def json_objects(text):
    """every JSON object in text, also when two ranks' lines ever share one line of the pipe"""
    dec, objs, i = json.JSONDecoder(), [], 0
    while True:
        i = text.find("{", i)
        if i < 0:
            return objs
        obj, i = dec.raw_decode(text, i)
        objs.append(obj)


def test_json_objects_parses_merged_lines():
    assert json_objects('noise\n{"rank": 0}{"rank": 1}\n\n{"rank": 2}\n') == [{"rank": 0}, {"rank": 1}, {"rank": 2}]


def test_gpus2_spawns_two_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--launch-check"],
                         capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = json_objects(out.stdout)
    assert sorted(l["rank"] for l in lines) == [0, 1]
    assert all(l["world_size"] == 2 for l in lines)


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_steps_outputs(tmp_path):
    """A plain run prints the headline fields only (what --full adds is absent), times exactly --steps rounds, and
    --dump-outputs holds what a caller reads back after the last timed round: the same workload stepped here, in this
    process, gives the same arrays, value for value (float64 holds every one of them exactly)."""
    import numpy as np
    import bench
    import swimsim

    n, warmup, steps = 4096, 6, 8
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--members", str(n), "--warmup",
                          str(warmup), "--steps", str(steps), "--dump-outputs", str(tmp_path)], env=env, cwd=REPO,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    lines = [l for l in json_objects(out.stdout) if "metric" in l]
    assert len(lines) == 1, out.stdout[-2000:]
    line = lines[0]
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert line["steps"] == steps and line["config"]["rounds_timed"] == steps
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(line["config"]["live_member_rounds"] / (line["ms_per_step"] * 1e-3 * steps),
                                          rel=1e-3)
    for key in ("roofline", "kernel_ms", "counters", "cpu_baseline", "hashring"):
        assert key not in line

    wl = bench.make_workload("config3", n, warmup + steps)
    eng = bench.new_cluster(swimsim, wl, 0, None)
    try:
        eng.step(warmup + steps, wl.events)
        got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in sorted(os.listdir(tmp_path))}
        assert all(a.dtype == np.float64 for a in got.values())
        assert sum(a.nbytes for a in got.values()) <= 64 * 1000 * 1000
        assert eng.counters()["rounds"] == warmup + steps == got["counters"][sorted(eng.counters()).index("rounds")]
        assert (got["checksums"] == eng.checksums()).all() and got["checksums"].shape == (n,)
        assert (got["last_targets"] == eng.last_targets()).all()
        assert (got["counters"] == [eng.counters()[k] for k in sorted(eng.counters())]).all()
        assert [int(h) for h in got["digest"]] == [h for d in eng.digest() for h in (d >> 32, d & 0xFFFFFFFF)]
        assert got["rows_observers"].shape == (bench.DUMP_ROWS,)
        for i, o in enumerate(got["rows_observers"]):
            st, inc = eng.row(int(o))
            assert (got["rows_status"][i] == st).all() and (got["rows_incarnation"][i] == inc).all()
    finally:
        eng.close()


def test_live_member_rounds_counts_live_members_only():
    sys.path.insert(0, REPO)
    import bench
    from swimsim import workloads as W

    wl = W.config3(n=1000, rounds=30, kill_round=10)
    # rounds 5-24: 5 rounds of 1000 live members, then 15 rounds of 990
    assert bench.live_member_rounds(wl, 5, 24) == 5 * 1000 + 15 * 990
