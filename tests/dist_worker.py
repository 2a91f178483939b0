"""One shard of a sharded cluster in its own process (spawned by tests/test_dist_gpu.py).

Ranks attach through swimsim.dist.GlooTransport (torch.distributed gloo), so every collective exchange
between shard processes runs the same call sequence as the RCCL transport, on one GPU. Rank 0 checks
every round against the CPU oracle: all checksums, the canonical state digests, the phase-S targets and
the protocol counters, bit for bit. Exit code 0 = parity held.

The argument is a workload's name, or `incarnation:<scenario>` for a scenario of tests/incarnation_scenarios.py, whose
raw writes each rank makes on the observers it owns (incarnation_scenario below).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "ringpop-go_amd"))


def main():
    import numpy as np
    import torch.distributed as dist
    import swimsim
    from swimsim import dist as sd
    from swimsim import workloads as W

    dist.init_process_group("gloo")
    ws, rank = dist.get_world_size(), dist.get_rank()
    name = sys.argv[1]
    if name.startswith("incarnation:"):
        sys.exit(incarnation_scenario(name.split(":", 1)[1], ws, rank))
    wl = {"config1": lambda: W.config1(), "config2": lambda: W.config2(n=128, rounds=40),
          "config4": lambda: W.config4(n=64, rounds=100, split_until=40, heals=(40, 60)),
          "config5": lambda: W.config5(n=96, rounds=45, every=15)}[name]()
    eng = swimsim.Cluster(wl.n, device=0, comm=(ws, rank, sd.GlooTransport()))
    ora = None
    if rank == 0:
        from oracle_ffi import OracleSim
        ora = OracleSim(wl.n)
    bad = 0
    for r in range(wl.rounds):
        ev = wl.events_for(r)
        eng.step(1, ev)
        cs = sd.gather_rows(eng.checksums())
        tg = sd.gather_rows(eng.last_targets())
        dg = sd.reduce_digest(eng.digest())
        ct = sd.reduce_counters(eng.counters())
        if rank == 0:
            ora.step(ev)
            ok = (cs == ora.checksums()).all() and (tg == ora.last_targets()).all() and dg == ora.digest() \
                and ct == ora.counters()
            if not ok:
                print(f"{name} round {r}: divergence (checksums {(cs != ora.checksums()).sum()} differ)", flush=True)
                bad = 1
        flag = [bad]
        dist.broadcast_object_list(flag, src=0)
        if flag[0]:
            break
    info = eng.shard_info()
    if rank == 0 and not bad:
        print(f"{name}: {wl.rounds} rounds bit-exact over {ws} processes, exchanges {info['exchanges']}", flush=True)
    eng.close()
    dist.destroy_process_group()
    sys.exit(bad)


def incarnation_scenario(name, ws, rank):
    """`incarnation:<scenario>` (tests/incarnation_scenarios.py, n = 65): a raw write is made on the rank that owns the
    observer, collective calls on every rank. Every rank steps an oracle of its own: it compares its writes' return
    values, after the last round its own observers' rows, dissemination buffers, timers and node statistics, and
    every round, together with the other ranks, what the workload runs compare. Returns the exit code (0 = parity)."""
    import numpy as np
    import torch.distributed as dist
    import swimsim
    import incarnation_scenarios as S
    from oracle_ffi import OracleSim
    from swimsim import dist as sd

    sc = S.scenario(name, 65)
    n = sc["n"]
    eng = swimsim.Cluster(n, device=0, comm=(ws, rank, sd.GlooTransport()), **sc["engine_kw"])
    ora = OracleSim(n, **sc["oracle_kw"])
    mine = range(eng.lo, eng.lo + eng.nl)

    def agreed(what):
        """None when no rank reports a difference, else the first report (every rank calls this)"""
        parts = [None] * ws
        dist.all_gather_object(parts, what)
        return next((p for p in parts if p), None)

    def compare_round(r):
        cs = sd.gather_rows(eng.checksums())
        tg = sd.gather_rows(eng.last_targets())
        dg = sd.reduce_digest(eng.digest())
        ct = sd.reduce_counters(eng.counters())
        if (cs == ora.checksums()).all() and (tg == ora.last_targets()).all() and dg == ora.digest() and ct == ora.counters():
            return None
        return f"round {r}: divergence (checksums of {np.nonzero(cs != ora.checksums())[0][:8]} differ)"

    bad = None
    for i, seg in enumerate(sc["segments"]):
        diff = None
        for op in seg["muts"]:
            want = S.apply(ora, op)
            if op[0] not in S.OWNED or op[1] in mine:
                got = S.apply(eng, op)
                if op[0] in S.COMPARED_RETURNS and got != want and diff is None:
                    diff = f"segment {i}: {op[0]} of observer {op[1]} returned {got}, the oracle {want}"
        bad = agreed(diff)
        r0 = eng.round
        for r in range(r0, r0 + seg["rounds"]):
            if bad:
                break
            if not seg.get("one_call"):
                eng.step(1, [e for e in seg["events"] if e[0] == r])
            elif r == r0:
                eng.step(seg["rounds"], seg["events"])
            ora.step([e for e in seg["events"] if e[0] == r])
            if not seg.get("one_call") or r == r0 + seg["rounds"] - 1:
                bad = agreed(compare_round(r))
        if bad:
            break
    if not bad:
        diff = None
        for o in mine:
            want = {"pingable": ora.num_pingable(o), "maxp": ora.maxp(o), "changes": ora.changes_count(o),
                    "members": ora.num_members(o)}
            est, einc = eng.row(o)
            ost, oinc = ora.row(o)
            if not ((est == ost).all() and (einc == oinc).all() and eng.changes(o) == ora.dis_entries(o) and
                    eng.timers(o) == ora.timer_entries(o) and eng.node_stats(o) == want):
                diff = f"at the end: observer {o} (row, dissemination, timers or node_stats) differs"
                break
        bad = agreed(diff)
    if rank == 0:
        if bad:
            print(f"incarnation:{name}: {bad}", flush=True)
        else:
            print(f"incarnation:{name}: {ora.round} rounds bit-exact over {ws} processes, final state of every observer "
                  f"included, exchanges {eng.shard_info()['exchanges']}", flush=True)
    eng.close()
    dist.destroy_process_group()
    return 1 if bad else 0


if __name__ == "__main__":
    main()
