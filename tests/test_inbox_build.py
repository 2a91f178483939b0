"""The receive phases' inboxes, built by counting: a key takes a slot of its receiver's run, one
launch scans the run sizes, and k_pair_info ranks every sender value inside its run. The order inside a run is what
the protocol sees (a receiver merges its messages in sender order), so every case runs against the oracle every
round with test_engine_parity's comparison: targets, checksums, digests, and the counters at the end.

The cases are the shapes at which the build takes another path: runs longer than a workgroup and no multiple of
a wave (ranked by whole waves), ping-req values o * K + q with several per receiver, inboxes of sentinels only,
a row count that is an exact multiple of the wave, and keys imported from other shards in arrival order."""
import numpy as np
import pytest

import swimsim
from swimsim import workloads as W
from test_engine_parity import make_pair, run_parity
from test_sharded_parity import make_sharded

pytestmark = pytest.mark.gpu


def seed(wl, eng, ora=None):
    """the workload's MakeChange seeding before round 0"""
    for o in range(wl.n):
        for m in wl.seed_members:
            if m != o:
                eng.make_change(o, m, swimsim.T0_MS, swimsim.ALIVE)
                if ora is not None:
                    ora.make_change(o, m, swimsim.T0_MS, 0)


SELFSTART = dict(n=2500, seeds=2, rounds=12)


def test_selfstart_long_inboxes_in_sender_order():
    """every node pings one of the two seeds: each seed's inbox holds about 1,250 messages, each from another
    source with its own content, so any other order inside the run changes what the seed's row becomes"""
    wl = W.selfstart(**SELFSTART)
    eng, ora = make_pair(wl.n, init="self")
    seed(wl, eng, ora)
    run_parity(eng, ora, wl.n, wl.rounds)
    assert ora.counters()["full_syncs"] > 0


def test_pingreq_inboxes():
    n = 192
    eng, ora = make_pair(n)
    ev = [(2, W.EV_KILL, m, 0) for m in range(0, n, 2)]
    run_parity(eng, ora, n, 40, ev)
    c = ora.counters()
    assert c["pingreqs"] > 0 and c["helper_calls"] > 0


def test_empty_inboxes():
    """one live member: no pingable target, so both phases' keys are all sentinels and every run is empty"""
    n = 65
    eng, ora = make_pair(n)
    ev = [(1, W.EV_KILL, m, 0) for m in range(1, n)]
    run_parity(eng, ora, n, 10, ev)


def test_rows_an_exact_multiple_of_the_wave():
    n = 64
    eng, ora = make_pair(n)
    run_parity(eng, ora, n, 5)


def test_sharded_imported_keys():
    """three shards: a seed's inbox is mostly keys that other shards sent, appended in arrival order"""
    wl = W.selfstart(n=333, seeds=2, rounds=25)
    eng, ora = make_sharded(wl.n, 3, init="self")
    seed(wl, eng, ora)
    run_parity(eng, ora, wl.n, wl.rounds)
    assert ora.counters()["full_syncs"] > 0


def test_selfstart_twice_is_the_same_round_for_round():
    """the slots inside a run come from atomics; the ranks must hide their order"""
    wl = W.selfstart(**SELFSTART)
    runs = []
    for _ in range(2):
        eng = swimsim.Cluster(wl.n, init="self")
        seed(wl, eng)
        rec = []
        for _r in range(wl.rounds):
            eng.step(1)
            rec.append((eng.checksums().copy(), tuple(eng.digest())))
        runs.append(rec)
        eng.close()
    for r, (a, b) in enumerate(zip(*runs)):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1], f"round {r}"
