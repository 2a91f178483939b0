"""CPU side of the address-width tests: the oracle's checksum string at every address width W = 13..20 and every
record-length regime of tests/address_scenarios.py against a plain Python join of its rows
(memberlist.go:106-128), and swimsim_create's address checks, which return before any device call. The GPU tests
(tests/test_address_widths.py) trust the oracle at exactly these widths and regimes."""
import ctypes

import numpy as np
import pytest

import address_scenarios as S
from oracle_ffi import fingerprint32

N = 130
# the round counts the GPU tests run the scenario for (kernel sweep and in-round paths, round parity)
ROUNDS = (12, 15)


@pytest.mark.parametrize("regime", sorted(S.REGIMES))
def test_scenario_covers_statuses_and_digit_counts(regime):
    """after each round count the GPU tests use, the oracle's rows hold all five statuses and, in the regimes that
    cross a digit boundary, incarnations of at least two digit counts"""
    for n in (N, 1100):
        ora, start, ev = S.make_oracle(n, 14, regime)
        for r in range(start, start + max(ROUNDS)):
            ora.step([e for e in ev if e[0] == r])
            if r + 1 - start in ROUNDS:
                S.check_coverage(ora, regime)
    statuses, digits = S.coverage(ora)
    want = {"A": {13}, "B": {13, 14}, "C": {15, 16}, "D": {1, 2, 3}}[regime]
    assert digits == want, digits


@pytest.mark.parametrize("regime", sorted(S.REGIMES))
@pytest.mark.parametrize("w", S.WIDTHS)
def test_oracle_string_is_the_plain_join(w, regime):
    scheme = w & 1
    ora = S.run_oracle(N, w, regime, 12, scheme)
    addrs = S.addresses(N, w, scheme)
    st, inc = ora.rows()
    cs = ora.checksums()
    lens = set()
    for o in range(N):
        want = S.python_checksum_string(addrs, st[o], inc[o])
        assert ora.checksum_string(o) == want, f"observer {o}"
        assert fingerprint32(want) == int(cs[o]), f"observer {o}"
        lens.add(len(want))
    assert len(lens) > 1                                 # the rows are not all alike


def test_record_extremes_occur():
    """the scenario reaches both ends of the record table: a 44-byte record (W = 20, suspect, 16 digits) and a
    20-byte one (W = 13, alive, 1 digit)"""
    for rounds in ROUNDS:
        ora = S.run_oracle(N, 20, "C", rounds)
        st, inc = ora.rows()
        assert ((st == 1) & (inc >= 10**15)).any()        # 20 + len("suspect") + 16 + 1 = 44
        ora = S.run_oracle(N, 13, "D", rounds)
        st, inc = ora.rows()
        assert ((st == 0) & (inc < 10)).any()             # 13 + len("alive") + 1 + 1 = 20


def test_burst_scenario_has_rounds_of_1024_distinct_changed_rows():
    """the in-round test of the reference-row path needs a launch of at least 1,024 rows after the engine has grouped
    equal rows: with the burst, some round of the 12 changes at least 1,024 of the 1,100 rows into distinct rows"""
    n = 1100
    ora, start, _ = S.make_oracle(n, 14, "B")
    _, _, ev = S.scenario(n, "B", burst=0.1)
    prev, best = ora.checksums().copy(), 0
    for r in range(start, start + 12):
        ora.step([e for e in ev if e[0] == r])
        cs = ora.checksums()
        best = max(best, len(set(cs[cs != prev].tolist())))
        prev = cs.copy()
    assert best >= 1024, best


def _create_rc(addrs, n=None):
    import swimsim
    L = swimsim.load_library()
    n = len(addrs) if n is None else n
    cfg = swimsim.make_config(n)
    cfg._addr_buf, cfg.addr_stride = swimsim.pack_addresses(addrs)
    cfg.addresses = ctypes.cast(cfg._addr_buf, ctypes.c_char_p)
    h = ctypes.c_void_p()
    rc = L.swimsim_create(ctypes.byref(cfg), ctypes.byref(h))
    assert not h.value
    return rc


@pytest.mark.parametrize("case", ["width12", "width21", "unequal", "equal_neighbours", "descending"])
def test_create_rejects_addresses_without_touching_device(case):
    a = S.addresses(8, 14)
    if case == "width12":
        a = [x[2:] for x in a]
    elif case == "width21":
        a = ["0000000" + x for x in a]
    elif case == "unequal":
        a[5] = a[5][1:]
    elif case == "equal_neighbours":
        a[4] = a[3]
    elif case == "descending":
        a[2], a[3] = a[3], a[2]
    assert _create_rc(a) == -1                             # SWIMSIM_EINVAL


def test_make_config_and_sharded_cluster_take_addresses():
    """make_config passes addresses through (ShardedCluster builds its shards from it): the packed buffer lives with
    the config, and a wrong count is an error"""
    import swimsim
    a = S.addresses(8, 14)
    cfg = swimsim.make_config(8, addresses=a)
    assert cfg.addr_stride == 14
    assert ctypes.string_at(cfg.addresses, 8 * 14) == "".join(a).encode()
    assert swimsim.make_config(8).addresses is None
    with pytest.raises(ValueError):
        swimsim.make_config(9, addresses=a)
    # a sharded cluster's bad addresses are refused (before any device call), not dropped
    bad = list(a)
    bad[2], bad[3] = bad[3], bad[2]
    with pytest.raises(swimsim.SwimsimError, match="EINVAL"):
        swimsim.ShardedCluster(8, 2, addresses=bad)
