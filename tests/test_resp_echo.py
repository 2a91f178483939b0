"""Echoed response records on the MI355X engine (swimsim_tuning.resp_echo) against the CPU oracle.

A receiver leaves out of its ping or ping-req response every record that only repeats what the sender's message has just
told it. Nothing may change but the records written: every shape of tests/resp_echo_cases.py runs with the path on
and off, one round per step call, and after every round the checksums, the three state digests, the ping targets and
the 18 counters are compared with the oracle's; at the end the words, dissemination cells and timers of sampled rows.
The two engine runs are then equal in every read-back, and the measurement counters must add up:
resp_merged(off) == resp_merged(on) + resp_echoed(on), recv_issued equal, resp_echoed(off) == 0. Everything is
integer work: the bar is bit-exact. tests/test_resp_echo_host.py shows on the oracle what each shape reaches.
"""
import functools

import numpy as np
import pytest

import fuzz_scenarios as F
import resp_echo_cases as R
import swimsim
from oracle_ffi import OracleSim
from test_fuzz import run_case

pytestmark = pytest.mark.gpu

SHAPES = {f"cascade-{n}-{k}": (n, R.cascade_events(n, k), {}, R.CASCADE_OPTS) for n, k in R.CASCADES}
SHAPES.update(R.WALKS)
COLD = [s for s in SHAPES if s.startswith("cold")]


def sampled(n):
    """first, last, the rows around a 64-row boundary and a few killed and live ones in between"""
    return sorted({0, 1, 2, 63, 64, 65, n // 2, n - 2, n - 1} & set(range(n)))


def read_round(sim):
    return (sim.checksums().tobytes(), tuple(sim.digest()), sim.last_targets().tobytes(),
            tuple(sorted(sim.counters().items())))


def read_end(sim, n, oracle):
    out = []
    for o in sampled(n):
        st, inc = sim.row(o)
        out.append((o, st.tobytes(), np.asarray(inc, np.int64).tobytes(),
                    sim.dis_entries(o) if oracle else sim.changes(o), sim.timer_entries(o) if oracle else sim.timers(o)))
    return out


@functools.lru_cache(maxsize=None)
def oracle_trace(shape):
    n, ev, _, opts = SHAPES[shape]
    ora = OracleSim(n, **opts)
    rounds = []
    for r in range(R.ROUNDS):
        ora.step([e for e in ev if e[0] == r])
        rounds.append(read_round(ora))
    return rounds, read_end(ora, n, True)


@functools.lru_cache(maxsize=None)
def engine_trace(shape, echo, shards=1):
    """(per-round read-backs, sampled rows at the end, kernel_units()) of one engine run"""
    n, ev, tuning, opts = SHAPES[shape]
    tuning = dict(tuning, resp_echo=echo)
    eng = swimsim.Cluster(n, tuning=tuning, **opts) if shards == 1 else swimsim.ShardedCluster(n, shards, tuning=tuning, **opts)
    try:
        rounds = []
        for r in range(R.ROUNDS):
            eng.step(1, [e for e in ev if e[0] == r])
            rounds.append(read_round(eng))
        return rounds, read_end(eng, n, False), eng.kernel_units()
    except swimsim.SwimsimError as e:
        if "EHIP" in str(e):                                        # a device error: nothing more runs on this GPU
            pytest.exit(f"{shape} resp_echo {echo} shards {shards}: device error, the session ends here: {e}", returncode=3)
        raise
    finally:
        eng.close()


def assert_same(got, want, label, what):
    (grounds, gend), (wrounds, wend) = got, want
    names = ("checksums", "digest", "targets", "counters")
    for r, (g, w) in enumerate(zip(grounds, wrounds)):
        for k, name in enumerate(names):
            if g[k] != w[k]:
                detail = f"{g[k]} vs {w[k]}" if name in ("digest", "counters") else ""
                pytest.fail(f"{label}: round {r}: {name} differ from {what} {detail}")
    for g, w in zip(gend, wend):
        for k, name in enumerate(("observer", "status", "incarnations", "dissemination cells", "timers")):
            assert g[k] == w[k], f"{label}: at the end: {name} of row {g[0]} differ from {what}"


def assert_identity(on, off, label, expect_echoes=True):
    print(f"{label}: on  { {k: int(on[k]) for k in ('recv_issued', 'resp_merged', 'resp_echoed')} }\n"
          f"{label}: off { {k: int(off[k]) for k in ('recv_issued', 'resp_merged', 'resp_echoed')} }")
    assert off["resp_echoed"] == 0
    assert on["recv_issued"] == off["recv_issued"]
    assert off["resp_merged"] == on["resp_merged"] + on["resp_echoed"]
    assert (on["resp_echoed"] > 0) == expect_echoes


@pytest.mark.parametrize("echo", [1, 0])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_engine_matches_oracle(shape, echo):
    rounds, end, _ = engine_trace(shape, echo)
    assert_same((rounds, end), oracle_trace(shape), f"{shape} resp_echo {echo}", "the oracle")


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_on_equals_off_and_the_counters_add_up(shape):
    on, off = engine_trace(shape, 1), engine_trace(shape, 0)
    assert_same(on[:2], off[:2], shape, "the run with resp_echo 0")
    assert_identity(on[2], off[2], shape, expect_echoes=shape not in COLD)   # (no hot slots: nothing may be skipped)


def test_ping_req_responses_are_merged_by_several_helpers_per_sender():
    ctr = dict(oracle_trace("pingreq-130")[0][-1][3])
    assert ctr["helper_calls"] > 2 * ctr["pingreqs"] > 0, ctr


@pytest.mark.parametrize("shards", [2, 3])
@pytest.mark.parametrize("n,k", R.SHARDED, ids=[f"{n}-{k}" for n, k in R.SHARDED])
def test_sharded(n, k, shards):
    """imported records are re-tagged with the receiving shard's slots, and responses are exported"""
    shape = f"cascade-{n}-{k}"
    on, off = engine_trace(shape, 1, shards), engine_trace(shape, 0, shards)
    assert_same(on[:2], oracle_trace(shape), f"{shape} over {shards} shards, resp_echo 1", "the oracle")
    assert_same(off[:2], oracle_trace(shape), f"{shape} over {shards} shards, resp_echo 0", "the oracle")
    assert_identity(on[2], off[2], f"{shape} over {shards} shards")
    one = engine_trace(shape, 1)[2]
    assert on[2]["recv_issued"] == one["recv_issued"]              # the same responses as on one shard


# ---- the two exclusions: tombstone records (evicted members still buffered) and the sender's own member (a refute on
# a stepped-back clock), in seeded random schedules that reach them (tests/test_resp_echo_host.py) ----
def run_fuzz(n, seed, echo):
    c = F.case(n, seed)
    eng = swimsim.Cluster(n, init=c["init"], tuning={"resp_echo": echo}, **c["options"])
    ora = OracleSim(n, init=c["init"], **c["options"])
    try:
        run_case(eng, ora, c, f"case {n}-{seed} resp_echo {echo}")
        return eng.kernel_units()
    finally:
        eng.close()


@pytest.mark.parametrize("n,seed", R.EXCLUSIONS, ids=[f"{n}-{s}" for n, s in R.EXCLUSIONS])
def test_exclusions_in_random_schedules(n, seed):
    on, off = run_fuzz(n, seed, 1), run_fuzz(n, seed, 0)
    assert_identity(on, off, f"case {n}-{seed}")


def test_the_switch_is_validated():
    with pytest.raises(swimsim.SwimsimError):
        swimsim.Cluster(8, tuning={"resp_echo": 2})
