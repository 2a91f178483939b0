"""Canonical records of a fuzz schedule's run (tests/fuzz_scenarios.py), taken the same way from the CPU oracle and
from the engine, so that both sides hash the same bytes. TEST INFRASTRUCTURE ONLY.

tests/golden/make_fuzz_fixtures.py writes the oracle's records of the mass schedules to tests/golden/fuzz_mass_*.json,
tests/test_fuzz_at_size_host.py regenerates them on the single-threaded oracle, tests/test_fuzz_at_size.py compares the
MI355X engine with them.

call_record(sim, c, rets): after the last round of a step call: sha256 of the checksum vector (<u4) and of the last
  ping targets (<i4), the three state digests, the counters, converged(), the compared mutator returns (make_change,
  add_join_list, the target list of a direct heal), and for each watched observer the number of events (applying
  Updates) and of changes since the last call (at most 4 n, which the logs of both sides hold), the sha256 of the
  stream and (old checksum, new checksum, NumMembers). The stream is serialised as little-endian integers: per Update
  a <u4 count, then per change <i4 member, <i4 status, <i8 incarnation, <i4 source, <i8 source incarnation; the changes
  of one Update in member order.
final_record(sim, c): sha256 of rows() status (u1) and incarnations (<i8), of every observer's iterator state (<i8
  index, <u4 epoch), of its node statistics (<i4 pingable, maxp, changes, members), of the clock offsets (<i8), and of
  every observer's dissemination entries (<u4 count, then the columns <i4 member, <i4 p, <i4 source, <i8 source
  incarnation, each in member order) and timer entries (<u4 count, then the columns <i4 member, <i4 state, <i4 fired,
  <i8 deadline, <i8 subject incarnation), observers in order.
"""
import collections
import ctypes as C
import hashlib
import struct
import time

import numpy as np

import fuzz_scenarios as F

UNKNOWN = F.UNKNOWN


def sha(a, dt):
    return hashlib.sha256(np.ascontiguousarray(a).astype(dt).tobytes()).hexdigest()


def is_oracle(sim):
    return hasattr(sim, "drain_events")


def drain(sim, o):
    """the per-Update stream of watched observer o since the last drain, one Update's changes in member order"""
    if is_oracle(sim):
        ev, old, new, nm = sim.drain_events(o)
        return [sorted(x) for x in ev], old, new, nm
    return sim.applied_events(o)


def stream_bytes(events):
    out = []
    for changes in events:
        out.append(struct.pack("<I", len(changes)))
        out += [struct.pack("<iiqiq", *ch) for ch in changes]
    return b"".join(out)


def plain(x):
    """mutator returns as JSON holds them"""
    return [plain(v) for v in x] if isinstance(x, (list, tuple)) else int(x)


def call_record(sim, c, call, rets):
    watch = {}
    for o in c["watch"]:
        ev, old, new, nm = drain(sim, o)
        changes = sum(len(x) for x in ev)
        assert changes <= 4 * c["n"], f"the stream of {o} fills its log ({changes} changes): shorten the call"
        watch[str(o)] = {"events": len(ev), "changes": changes, "checksums_members": [int(old), int(new), int(nm)],
                         "stream_sha256": hashlib.sha256(stream_bytes(ev)).hexdigest()}
    return {"round": call["round"] + call["rounds"] - 1, "checksums_sha256": sha(sim.checksums(), "<u4"),
            "targets_sha256": sha(sim.last_targets(), "<i4"), "digest": [f"{x:016x}" for x in sim.digest()],
            "counters": {k: int(v) for k, v in sim.counters().items()}, "converged": bool(sim.converged()),
            "returns": plain(rets), "watch": watch}


class _Columns:
    """every observer's dissemination and timer entries as columns in member order, read by the C calls behind
    dis_entries / changes and timer_entries / timers (whose Python dicts take seconds to build at 4,160 members)"""

    def __init__(self, sim, n):
        self.n = n
        self.i4 = [np.empty(n, np.int32) for _ in range(3)]
        self.i8 = [np.empty(n, np.int64) for _ in range(2)]
        if is_oracle(sim):
            import oracle_ffi
            L = oracle_ffi.lib()
            self.dis = lambda o: L.or_dis_entries(sim.h, o, *self.ptrs(3, 1), n)
            self.tim = lambda o: L.or_timer_entries(sim.h, o, *self.ptrs(3, 2), n)
        else:
            L = swimsim_library()
            self.k = C.c_size_t()
            own = sim.owner if hasattr(sim, "owner") else (lambda o: sim)
            self.dis = lambda o: self.engine(own(o), L.swimsim_changes, o, 1)
            self.tim = lambda o: self.engine(own(o), L.swimsim_timers, o, 2)

    def ptrs(self, a, b):
        return [x.ctypes.data for x in self.i4[:a] + self.i8[:b]]

    def engine(self, cl, fn, o, wide):
        cl._chk(fn(cl.h, o, *self.ptrs(3, wide), self.n, C.byref(self.k)))
        return self.k.value

    def hashed(self, h, k, wide):
        assert 0 <= k <= self.n
        h.update(struct.pack("<I", k))
        for x in self.i4 + self.i8[:wide]:
            h.update(x[:k].astype(x.dtype.newbyteorder("<")).tobytes())


def swimsim_library():
    import swimsim
    return swimsim.load_library()


def final_record(sim, c):
    n = c["n"]
    st, inc = sim.rows()
    ora = is_oracle(sim)
    cols = _Columns(sim, n)
    it, stats, dis, tim = [], [], hashlib.sha256(), hashlib.sha256()
    for o in range(n):
        it.append(struct.pack("<qI", *sim.iter_state(o)))
        if ora:
            ns = (sim.num_pingable(o), sim.maxp(o), sim.changes_count(o), sim.num_members(o))
        else:
            s = sim.node_stats(o)
            ns = (s["pingable"], s["maxp"], s["changes"], s["members"])
        stats.append(struct.pack("<4i", *ns))
        cols.hashed(dis, cols.dis(o), 1)
        cols.hashed(tim, cols.tim(o), 2)
    return {"status_sha256": sha(st, "u1"), "incarnations_sha256": sha(inc, "<i8"),
            "iterators_sha256": hashlib.sha256(b"".join(it)).hexdigest(),
            "node_stats_sha256": hashlib.sha256(b"".join(stats)).hexdigest(),
            "clock_offsets_sha256": sha(sim.clock_offsets(), "<i8"),
            "dissemination_sha256": dis.hexdigest(), "timers_sha256": tim.hexdigest()}


def start_watching(sim, c):
    for o in c["watch"]:
        sim.watch(o, "events")


def oracle_records(c, reach=False, upto=None, make=None):
    """the schedule on the CPU oracle: (oracle, {"calls": [call_record], "final": final_record}, reach block or None).
    reach=True snapshots rows() around every round (what the run reached: cells evicted by timers, the most cells one
    observer changed in one round). upto=k stops after call k, without a final record. make(n, **kw) builds the oracle."""
    if make is None:
        from oracle_ffi import OracleSim as make
    n = c["n"]
    ora = make(n, init=c["init"], **c["options"])
    start_watching(ora, c)
    got = {"evicted": 0, "evicted_member_max": -1, "evicting_observer_max": -1, "row_changes_max": 0,
           "row_changes_observer": -1, "row_changes_round": -1}
    snap = {}

    def before_round(r):
        if snap.get("r") != r:                                     # (the first round, or mutators ran since)
            snap["st"], snap["inc"] = ora.rows()

    def after_round(r):
        st, inc = ora.rows()
        ev = (snap["st"] != UNKNOWN) & (st == UNKNOWN)             # turned UNKNOWN inside a round: evicted by a timer
        if ev.any():
            got["evicted"] += int(ev.sum())
            got["evicted_member_max"] = max(got["evicted_member_max"], int(np.nonzero(ev.any(axis=0))[0].max()))
            got["evicting_observer_max"] = max(got["evicting_observer_max"], int(np.nonzero(ev.any(axis=1))[0].max()))
        per = ((snap["st"] != st) | (snap["inc"] != inc)).sum(axis=1)
        if int(per.max()) > got["row_changes_max"]:
            got.update(row_changes_max=int(per.max()), row_changes_observer=int(per.argmax()), row_changes_round=r)
        snap.update(st=st, inc=inc, r=r + 1)

    t0 = time.time()
    recs = []
    for i, call in enumerate(c["calls"]):
        if call["muts"]:
            snap.pop("r", None)
        rets = F.oracle_call(ora, call, before_round if reach else None, after_round if reach else None)
        recs.append(call_record(ora, c, call, rets))
        if upto is not None and i == upto:
            return ora, {"calls": recs}, None
    out = {"calls": recs, "final": final_record(ora, c)}
    if not reach:
        return ora, out, None
    got["counters"] = ora.counters()
    got["events"] = dict(collections.Counter(F.EVENT_NAMES[e[1]] for call in c["calls"] for e in call["events"]))
    got["mutators"] = dict(collections.Counter(m[0] for call in c["calls"] for m in call["muts"]))
    got["oracle_seconds"] = round(time.time() - t0, 1)
    return ora, out, got
