"""Scenarios of the address-width tests (tests/test_address_widths_host.py on the CPU oracle,
tests/test_address_widths.py engine against oracle). TEST INFRASTRUCTURE ONLY.

The membership checksum hashes addr ‖ status ‖ decimal(inc) ‖ ';' per member, so the checksum kernels see two
lengths: the address width W (13..20 bytes, a template parameter of every phase-C kernel) and the record tail
status ‖ decimal(inc) ‖ ';' (7..24 bytes, from the handle's incarnation table). The regimes below pick t0 and the
period so that a dozen rounds cross a digit-count boundary of t0 + e * period; the event list puts every status into
the rows, so every status word length occurs and tombstones are skipped.
"""
import numpy as np

from swimsim import workloads as W

WIDTHS = tuple(range(13, 21))
SEED = 29


def addresses(n, w, scheme=0):
    """n strictly ascending addresses of exactly w bytes. Scheme 0 ends in a port (the last partial word is all
    digits), scheme 1 in a dotted name (letters and a dot in the last partial word)."""
    if scheme == 0:
        out = [f"{m:0{w - 5}d}:7000" for m in range(n)]
    else:
        out = [f"n{m:0{w - 4}d}.io" for m in range(n)]
    assert all(len(a) == w for a in out) and all(a < b for a, b in zip(out, out[1:]))
    return out


def _regime(t0_ms, period_ms, start):
    kw = dict(period_ms=period_ms, suspect_ms=5 * period_ms, faulty_ms=8 * period_ms, tombstone_ms=6 * period_ms)
    if t0_ms is not None:
        kw["t0_ms"] = t0_ms
    return {"kw": kw, "start": start}


# incarnations are t0 + e * period for incarnation step e (the round of the change)
REGIMES = {
    "A": _regime(None, 200, 0),                   # 13 digits throughout: tails of 19..21 bytes
    "B": _regime(10**13 - 5 * 200, 200, 0),       # 13 -> 14 digits at e = 5: tails of 19..22 bytes
    "C": _regime(10**15 - 5 * 200, 200, 0),       # 15 -> 16 digits at e = 5: tails up to 24 bytes, the table's maximum
    "D": _regime(1, 1, 95),                       # 1 -> 2 -> 3 digits at e = 9 and e = 99: tails from 7 bytes, the minimum
}
# regimes whose final rows must hold at least two incarnation digit counts
MIXED_DIGITS = ("B", "C", "D")


def events(n, start, burst=0.0):
    """kill, revive, reincarnate, leave and reap events over rounds start .. start + 11. The rows then hold alive
    members of old and new incarnations, suspects (killed at +7 and +10), faulty members (killed at +2), leavers and
    tombstones (killed at +0, reaped at +7 .. +9, evicted six periods later). burst: that fraction of the members
    reincarnates at +5 as well, so that around +8 .. +10 nearly every row changes in every round and hardly two rows
    are equal (launches of about n distinct rows)."""
    pick = W.distinct_members(SEED, start, 21, 20, n)
    k0, k1, k2, lv, re0, re1, re2 = pick[0:4], pick[4:7], pick[7:9], pick[9:12], pick[12:14], pick[14:17], pick[17:20]
    reapers = [m for m in range(n) if m not in pick][:3]
    ev = [(0, W.EV_KILL, m, 0) for m in k0]
    ev += [(1, W.EV_LEAVE, m, 0) for m in lv[:2]] + [(1, W.EV_REINCARNATE, m, 0) for m in re0]
    ev += [(2, W.EV_KILL, m, 0) for m in k1]
    ev += [(6, W.EV_REINCARNATE, m, 0) for m in re1]
    ev += [(7, W.EV_KILL, re1[0], 0)]                 # suspects of the new incarnations: the longest records
    ev += [(7 + i, W.EV_REAP, o, 0) for i, o in enumerate(reapers)]
    ev += [(9, W.EV_REVIVE, k0[0], 0)]
    ev += [(10, W.EV_KILL, m, 0) for m in k2 + [re1[1]]] + [(10, W.EV_REINCARNATE, m, 0) for m in re2]
    ev += [(11, W.EV_LEAVE, lv[2], 0)]
    if burst:
        ev += [(5, W.EV_REINCARNATE, m, 0) for m in W.distinct_members(SEED, start, 23, int(n * burst), n)]
    return [(start + r, k, a, b) for (r, k, a, b) in ev]


def scenario(n, regime, burst=0.0):
    """(Cluster / OracleSim keyword arguments, start round, events) of a regime at n members"""
    reg = REGIMES[regime]
    return dict(reg["kw"]), reg["start"], events(n, reg["start"], burst)


def make_oracle(n, w, regime, scheme=0, **kw):
    from oracle_ffi import OracleSim
    okw, start, ev = scenario(n, regime)
    okw.update(kw)
    ora = OracleSim(n, addresses=addresses(n, w, scheme), **okw)
    if start:
        ora.set_round(start)
    return ora, start, ev


def run_oracle(n, w, regime, rounds, scheme=0):
    ora, start, ev = make_oracle(n, w, regime, scheme)
    for r in range(start, start + rounds):
        ora.step([e for e in ev if e[0] == r])
    return ora


def coverage(ora):
    """(statuses that occur in the oracle's rows, digit counts of the incarnations of the members in a checksum)"""
    st, inc = ora.rows()
    statuses = set(int(s) for s in np.unique(st))
    digits = set(len(str(int(i))) for i in np.unique(inc[st < 4]))
    return statuses, digits


def check_coverage(ora, regime):
    statuses, digits = coverage(ora)
    assert {0, 1, 2, 3, 4} <= statuses, f"regime {regime}: statuses {sorted(statuses)}"
    if regime in MIXED_DIGITS:
        assert len(digits) >= 2, f"regime {regime}: incarnation digit counts {sorted(digits)}"
    return statuses, digits


STATUS_WORDS = ("alive", "suspect", "faulty", "leave")


def python_checksum_string(addrs, st_row, inc_row):
    """memberlist.go:106-128 in plain Python: address + status + decimal incarnation + ';' of every member that is
    neither a tombstone nor unknown, in address order (= index order: the addresses ascend)"""
    return "".join(f"{addrs[m]}{STATUS_WORDS[int(st_row[m])]}{int(inc_row[m])};"
                   for m in range(len(addrs)) if st_row[m] < 4).encode()
