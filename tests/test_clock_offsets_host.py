"""Per-node clock offsets, the part that needs no GPU: libswimsim.so exports and binds swimsim_set_clock_offset,
swimsim_set_clock_offsets and swimsim_clock_offsets, they reject a NULL handle without touching a device, and the
scenario the GPU tests replay (clock_scenarios.py, scenario S) really exercises skew on the oracle."""
import ctypes
import os

import clock_scenarios as CS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "ringpop-go_amd", "swimsim", "libswimsim.so")
NEW = ("swimsim_set_clock_offset", "swimsim_set_clock_offsets", "swimsim_clock_offsets")


def test_library_exports_and_binding_has_the_clock_entry_points():
    import swimsim
    raw = ctypes.CDLL(LIB)
    missing = [n for n in NEW if not hasattr(raw, n)]
    assert not missing, missing
    L = swimsim.load_library(LIB)
    for n in NEW:
        f = getattr(L, n)
        assert f.restype is ctypes.c_int and f.argtypes, n
    assert swimsim.EV_CLOCK == 8 and swimsim.workloads.EV_CLOCK == 8
    for cls in (swimsim.Cluster, swimsim.ShardedCluster):
        for m in ("set_clock_offset", "set_clock_offsets", "clock_offsets"):
            assert callable(getattr(cls, m)), (cls.__name__, m)


def test_null_handle_is_einval_without_touching_a_device():
    import swimsim
    L = swimsim.load_library(LIB)
    buf = (ctypes.c_int64 * 4)()
    assert L.swimsim_set_clock_offset(None, 0, 0) == -1
    assert L.swimsim_set_clock_offsets(None, ctypes.cast(buf, ctypes.c_void_p)) == -1
    assert L.swimsim_set_clock_offsets(None, None) == -1
    assert L.swimsim_clock_offsets(None, ctypes.cast(buf, ctypes.c_void_p)) == -1
    assert L.swimsim_clock_offsets(None, None) == -1


def test_scenario_s_exercises_skew_on_the_oracle():
    """with its clock steps, S ends in a different state and refutes more often: the stepped-back node's refutes
    carry an incarnation below the rumour's, so the rumour comes back and is refuted again"""
    skewed, plain = CS.run_oracle_s(True), CS.run_oracle_s(False)
    assert skewed.digest() != plain.digest()
    rs, rp = skewed.counters()["refutes"], plain.counters()["refutes"]
    print(f"refutes: {rs} with S's clock steps, {rp} without")
    assert rs > rp


def test_scenario_s_forward_step_fires_several_timers_in_one_round():
    """node 3's forward step at round 78 finds pending timers with different deadlines: they fire in that round's
    phase T as separate one-change Updates (MakeFaulty / MakeTombstone), which is what the engine's event-stream
    order test needs"""
    from oracle_ffi import OracleSim, FAULTY, TOMBSTONE
    ora = OracleSim(CS.S_N, **CS.S_KW)
    ora.set_round(CS.S_START)
    ora.watch(3, "events")
    for r in range(CS.S_START, 79):
        for (o, k) in CS.S_CLOCKS.get(r, []):
            ora.set_clock_offset(o, k * CS.P)
        fired = ora.counters()["timers_fired"]
        ora.step([e for e in CS.S_EVENTS if e[0] == r])
        events = ora.drain_events(3)[0]
    timer_events = [e for e in events if len(e) == 1 and e[0][1] in (FAULTY, TOMBSTONE) and e[0][3] == 3]
    assert len(timer_events) >= 2, events
    assert ora.counters()["timers_fired"] - fired >= len(timer_events)
