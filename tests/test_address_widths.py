"""The checksum kernels at every address width and record length, engine against CPU oracle, bit for bit
(memberlist.go:83-128: Fingerprint32 of addr ‖ status ‖ decimal(inc) ‖ ';' of every member).

Every phase-C kernel is a template on the address width W (CS_W_CASES in csrc/swimsim_checksum.hip: 13..20 bytes) and
is launched in one of two geometries: the one specialised for W = 19 with 13-digit incarnations (tails of 19..21
bytes), and the general one for any tail of up to 24 bytes. The handles here are created with real addresses of each
width and with t0 / period settings whose incarnations change their digit count mid-run
(tests/address_scenarios.py; tests/test_address_widths_host.py pins the oracle at the same widths and regimes on the
CPU). Sizes are never multiples of 64.
"""
from contextlib import closing

import numpy as np
import pytest

import address_scenarios as S
from oracle_ffi import OracleSim
import swimsim
from swimsim import workloads as W
from test_engine_parity import run_parity

pytestmark = pytest.mark.gpu

WIDE_ONLY = {"cs_narrow_rows": 0, "cs_async": 0}        # every launch takes the wide kernel, on the main stream
REF_PATH = {"cs_ref": 2, "cs_async": 0}                  # every launch of 1,024 rows or more takes the reference-row path

# (W, regime): every width with 13-digit and 13 -> 14-digit incarnations (W = 19 with regime A is what every other
# test of the suite runs), the partial-word cases bW = 1, 0, 3, 0 with the longest and the shortest tails
CASES = ([(w, r) for w in S.WIDTHS for r in "AB" if (w, r) != (19, "A")] +
         [(w, r) for w in (13, 16, 19, 20) for r in "CD"])


def case_id(c):
    return f"W{c[0]}{c[1]}"


def make_pair(n, w, regime, scheme=0, tuning=None, burst=0.0, **extra):
    kw, start, ev = S.scenario(n, regime, burst)
    kw.update(extra)
    addrs = S.addresses(n, w, scheme)
    eng = swimsim.Cluster(n, addresses=addrs, tuning=tuning, **kw)
    ora = OracleSim(n, addresses=addrs, **{k: v for k, v in kw.items() if k != "max_rounds"})
    if start:
        eng.set_round(start)
        ora.set_round(start)
    return eng, ora, start, ev


def units(eng):
    u = eng.kernel_units()
    return np.array([u["cs_rows_wide"], u["cs_rows_narrow"]], dtype=np.int64)


# ---- 1. round parity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["production", "wide"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_round_parity(case, variant):
    """15 rounds of the scenario at 130 members: checksums, digests, ping targets and counters every round. The
    production tuning hashes these few rows with the narrow kernel, the second variant sends every launch to the wide
    one. The two variants use the two address schemes."""
    w, regime = case
    n = 130
    wide = variant == "wide"
    eng, ora, start, ev = make_pair(n, w, regime, scheme=int(wide), tuning=WIDE_ONLY if wide else None)
    with closing(eng):
        u0 = units(eng)
        run_parity(eng, ora, n, 15, ev)
        du = units(eng) - u0
        print(f"W{w} {regime} {variant}: rows hashed wide / narrow {du.tolist()}")
        assert du[0 if wide else 1] > 0 and du[1 if wide else 0] == 0, du   # the variant's kernel ran, alone


def test_last_member_tombstone_then_lower_member_applies():
    """the scenario at the synthetic 19-byte addresses and 13-digit incarnations (the specialised kernels): it kills
    the last member, 129, which is reaped at +7, so the rows' last included member is invalidated (DS::clast = -2, the
    kernels rescan it), and revives member 30 at +9. A change applied below the true last included member must not
    become the row's last member: the FarmHash prologue would hash member 30's record as the string's last 20 bytes."""
    n = 130
    kw, start, ev = S.scenario(n, "A")
    assert (0, W.EV_KILL, n - 1, 0) in ev and any(e[1] == W.EV_REVIVE and e[2] < n - 1 for e in ev)
    eng, ora = swimsim.Cluster(n, **kw), OracleSim(n, **kw)
    with closing(eng):
        run_parity(eng, ora, n, 15, ev)
        st, _ = ora.rows()
        assert (st[:, n - 1] >= 4).any()


# ---- 2. kernel sweep -------------------------------------------------------------------------------------------
def raw_writes(eng, ora, n, k):
    """the same few raw row writes on both sides (no gossip, no checksum): the stored checksums of these rows are stale
    afterwards. They touch the first, a middle and the last member, every status, and incarnations on both sides of
    the regimes' digit boundaries; k makes every call's values new."""
    r, t0, p = eng.round, eng.t0_ms, eng.period_ms
    writes = [(3, 0, swimsim.SUSPECT, r + 1 + k), (n - 1, n // 2, swimsim.FAULTY, 1 + k), (64, n - 1, swimsim.TOMBSTONE, r),
              (65, n - 1, swimsim.LEAVE, r + 2 + k), (n // 2, n - 2, swimsim.ALIVE, 2 + k), (0, n - 1, swimsim.SUSPECT, r + k)]
    for (o, m, st, e) in writes:
        eng.set_member(o, m, st, t0 + e * p)
        ora.set_member(o, m, st, t0 + e * p)
    return sorted({o for (o, _, _, _) in writes})


def run_mode(eng, ora, n, mode, k, reps=1):
    """raw writes, then bench_checksum `mode` over all rows (a warm-up launch and `reps` timed ones) and a read-back:
    returns (rows counted by the wide and narrow kernels during the launches, the reference-row path's launches and
    fallback rows during them). Asserts that the read-back hashed nothing (what it returns is what the mode's kernel
    stored) and that every checksum equals the oracle's."""
    stale = raw_writes(eng, ora, n, k)
    want = ora.checksums()
    u0, p0 = units(eng), eng.checksum_path_stats()
    eng.bench_checksum(n, mode, reps=reps)
    u1, p1 = units(eng), eng.checksum_path_stats()
    got = eng.checksums()
    u2, p2 = units(eng), eng.checksum_path_stats()
    assert (u2 == u1).all() and p2 == p1, f"mode {mode}: the read-back hashed rows itself ({u1} -> {u2})"
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"mode {mode}: {len(bad)} checksums differ, first rows {bad[:5]} (stale rows {stale})"
    return u1 - u0, p1["delta_launches"] - p0["delta_launches"], p1["fallback_rows"] - p0["fallback_rows"], p1["reasons"]


def check_mode(eng, ora, n, mode, k, label):
    reps = 1
    launches = reps + 1
    du, dl, fb, reasons = run_mode(eng, ora, n, mode, k, reps)
    print(f"{label} mode {mode}: rows wide / narrow {du.tolist()}, path launches {dl}, fallback rows {fb}, reasons {reasons}")
    if mode in (1, 4):
        assert du.tolist() == [launches * n, 0] and dl == 0
    elif mode == 2:
        assert du.tolist() == [0, launches * n] and dl == 0
    else:
        # the reference-row path: k_csr3 counts the rows it hashed itself with the wide kernel's counter, the rows it
        # leaves go to the narrow kernel
        assert dl == launches
        assert du[0] + du[1] == launches * n and du[1] == fb, (du, fb)
        assert du[0] > 0, f"the reference-row path hashed no row itself: {reasons}"
    return du


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_kernel_sweep(case):
    """1,100 members (18 wide workgroups, 69 narrow ones): 12 scenario rounds in parity, then each checksum kernel
    over all rows after raw writes, with the proof that its launches hashed the rows compared"""
    w, regime = case
    n = 1100
    eng, ora, start, ev = make_pair(n, w, regime, scheme=w & 1)
    with closing(eng):
        run_parity(eng, ora, n, 12, ev)
        side = eng.memory()["side_cap"] >= 4097                   # the side buffer set exists (csr_side_min)
        for k, mode in enumerate((1, 2, 4, 5, 6)):
            if mode == 6 and not side:
                with pytest.raises(swimsim.SwimsimError, match="unavailable"):
                    eng.bench_checksum(n, 6, reps=1)
                continue
            check_mode(eng, ora, n, mode, 3 * k, f"W{w} {regime}")
        assert eng.digest() == ora.digest()


# ---- 3. the narrow kernel at 8 records per step ------------------------------------------------------------------
@pytest.mark.parametrize("w", [13, 20])
def test_narrow_kernel_8_records_per_step(w):
    """more than 256 narrow row groups (4,096 rows): k_checksum_q16<..., 8>. 4,160 members, regime B, started at round
    5 so that the rounds' incarnations have 14 digits and the initial ones 13; three rounds with events, then the
    narrow kernel and (the side buffer set exists at this size) the side-stream reference-row path over all rows"""
    n = 4160
    kw, _, _ = S.scenario(n, "B")
    addrs = S.addresses(n, w, 1)
    with closing(swimsim.Cluster(n, addresses=addrs, **kw)) as eng:
        ora = OracleSim(n, addresses=addrs, **kw)
        eng.set_round(5)
        ora.set_round(5)
        pick = W.distinct_members(S.SEED, 5, 22, 12, n)
        ev = ([(5, W.EV_KILL, m, 0) for m in pick[:4]] + [(5, W.EV_REINCARNATE, m, 0) for m in pick[4:8]] +
              [(5, W.EV_LEAVE, m, 0) for m in pick[8:10]] + [(6, W.EV_REINCARNATE, m, 0) for m in pick[10:]])
        run_parity(eng, ora, n, 3, ev)
        check_mode(eng, ora, n, 2, 0, f"W{w} B n{n}")
        assert eng.memory()["side_cap"] >= 4097
        check_mode(eng, ora, n, 6, 3, f"W{w} B n{n}")
        st, inc = ora.row(0)
        assert len({len(str(int(i))) for i in inc[st < 4]}) == 2     # both digit counts in one row


# ---- 4. the reference-row path inside rounds ---------------------------------------------------------------------
@pytest.mark.parametrize("case", [(w, "B") for w in S.WIDTHS] + [(13, "C"), (20, "C")], ids=case_id)
def test_reference_row_path_in_rounds(case):
    """the scenario with a burst (a tenth of the members reincarnates at +5): around +8 .. +10 a round's launch holds
    more than 1,024 distinct rows, which the forced reference-row path takes (CSD_MIN_ROWS)"""
    w, regime = case
    n = 1100
    eng, ora, start, ev = make_pair(n, w, regime, scheme=w & 1, tuning=REF_PATH, burst=0.1)
    with closing(eng):
        u0 = units(eng)
        run_parity(eng, ora, n, 12, ev)
        du = units(eng) - u0
        st = eng.checksum_path_stats()
        print(f"W{w} {regime} in rounds: rows wide / narrow {du.tolist()}, {st}")
        assert st["delta_launches"] >= 1, st
        # cs_narrow_rows is the production 8,192, so no launch here takes the wide kernel: its counter holds the rows
        # the path hashed itself (k_csr3), the rows offered less the rows left to the production kernels
        assert du[0] > 0, f"the path left every row to the production kernels: {st}"
        assert du[1] >= st["fallback_rows"]


# ---- 5. table growth across a digit boundary ---------------------------------------------------------------------
@pytest.mark.parametrize("w", [19, 14])
def test_table_growth_across_digit_boundary(w):
    """max_rounds = 16 and t0 = 10^13 - 40 periods: the incarnation table is rebuilt at rounds 15 and 31, and the
    second rebuild brings the first 14-digit incarnation (e = 40), so the longest tail goes from 21 to 22 bytes and
    (W = 19) the launchers change from the specialised to the general kernels between two rounds"""
    n = 130
    kw, _, _ = S.scenario(n, "A")
    kw.update(t0_ms=10**13 - 40 * 200, max_rounds=16)
    addrs = S.addresses(n, w, 0)
    ev = S.events(n, 0) + S.events(n, 38)
    with closing(swimsim.Cluster(n, addresses=addrs, **kw)) as eng:
        ora = OracleSim(n, addresses=addrs, **{k: v for k, v in kw.items() if k != "max_rounds"})
        run_parity(eng, ora, n, 60, ev)
        _, digits = S.coverage(ora)
        assert digits == {13, 14}, digits


# ---- 6. sharded cluster ------------------------------------------------------------------------------------------
def test_sharded_cluster_with_addresses():
    n, w = 130, 14
    kw, start, ev = S.scenario(n, "B")
    addrs = S.addresses(n, w, 0)
    eng = swimsim.ShardedCluster(n, 3, addresses=addrs, **kw)
    with closing(eng):
        ora = OracleSim(n, addresses=addrs, **kw)
        run_parity(eng, ora, n, 12, ev)
        S.check_coverage(ora, "B")
        # (not the synthetic addresses' checksums: those were what a sharded cluster hashed before it took addresses)
        assert (OracleSim(n, **kw).checksums() != OracleSim(n, addresses=addrs, **kw).checksums()).all()


# ---- 7. refusals, never a wrong checksum -------------------------------------------------------------------------
def test_refuses_25_byte_tail():
    """t0 = 10^16 - 3 periods: "suspect" + 17 digits + ';' is 25 bytes"""
    with pytest.raises(swimsim.SwimsimError, match="swimsim_create failed: EINVAL"):
        swimsim.Cluster(130, addresses=S.addresses(130, 14), t0_ms=10**16 - 3 * 200)


def test_refuses_digit_count_jump():
    """t0 = 1 with a 200 ms period: 1, 201, ... the digit count jumps by two in one step"""
    with pytest.raises(swimsim.SwimsimError, match="swimsim_create failed: EINVAL"):
        swimsim.Cluster(130, addresses=S.addresses(130, 14), t0_ms=1, period_ms=200)


def test_refuses_string_of_20_bytes_and_next_handle_works():
    """one member, 13-byte address, incarnation 1: the whole string is 20 bytes, and FarmHash's paths for strings of
    at most 24 bytes are not implemented: an error, from init or the first step. A fresh default handle works."""
    kw = S.REGIMES["D"]["kw"]
    with pytest.raises(swimsim.SwimsimError, match=r"24.byte"):
        eng = swimsim.Cluster(1, addresses=S.addresses(1, 13), **kw)
        try:
            eng.step(1)
            eng.checksums()
        finally:
            eng.close()
    n = 130
    eng, ora = swimsim.Cluster(n), OracleSim(n)
    with closing(eng):
        run_parity(eng, ora, n, 3, [(0, W.EV_KILL, 5, 0)])
