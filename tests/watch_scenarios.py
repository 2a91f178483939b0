"""Scenarios for the edges of the applied-change streams (swimsim_watch, swimsim_applied_changes,
swimsim_applied_events): tests/test_watch_edges_host.py runs them on the CPU oracle alone and asserts that each reaches
the path it is written for, tests/test_watch_edges.py runs them engine against oracle. TEST INFRASTRUCTURE ONLY: pure
Python builders and constants, no GPU, no oracle import.

A  drains past one member per thread. The coalesced drain (k_drain_applied) is one workgroup of 1,024 threads; thread
   t takes the C = ceil(NP / 1024) consecutive members [t * C, min(t * C + C, N)), NP = N rounded up to 64, and a block
   scan of the threads' counts places the records in member order. Up to N = 1,024 that is one member per thread.
   JOIN    four AddJoinList calls on one observer of a converged cluster, no rounds: N - 1 changes, a seeded 40 %, the
           two end members, the last member. Sizes 1025 (C = 2, last run clipped to 1), 1100 (C = 2, threads 550..1023
           idle), 2100 (C = 3), 3073 (C = 4, last run clipped to 1).
   ROUNDS  12 protocol rounds after 30 % of the members reincarnate in round 1, three observers watched.
   FUZZ    two fuzz schedules (tests/fuzz_scenarios.py) at N = 1,100, a converged start and a self-only one.
B  the 64 watch slots of a handle at N = 130 under churn: all 64 taken, a 65th refused, a slot given up with changes
   still logged and taken again, an observer moved between the coalesced drain and the per-Update stream.
C  overflow of the per-Update log at N = 64: the log holds event_log_capacity(N) changes since the last drain.
D  caller buffers shorter than the drain, at N = 130 under churn.
"""
import random

from swimsim import workloads as W

ALIVE = 0
T0_MS = 1_500_000_000_000
PERIOD_MS = 200
EV_REINCARNATE = W.EV_REINCARNATE
DRAIN_THREADS = 1024                             # k_drain_applied's workgroup
WATCH_SLOTS = 64                                 # watched observers per handle (include/swimsim.h)


def padded(n):
    """NP: N rounded up to a multiple of 64"""
    return (n + 63) // 64 * 64


def run_length(n):
    """C: the members one thread of the coalesced drain takes"""
    return (padded(n) + DRAIN_THREADS - 1) // DRAIN_THREADS


def runs(n):
    """[(first member, end)] of the non-empty thread runs of the coalesced drain, in thread order"""
    c = run_length(n)
    return [(b, min(b + c, n)) for b in range(0, n, c)]


def run_fill(members, n):
    """per non-empty thread run of the coalesced drain: (run length, members of it in `members`)"""
    s = set(members)
    return [(e - b, sum(m in s for m in range(b, e))) for b, e in runs(n)]


def touched_runs(members, n):
    """indices of the thread runs that hold one of `members`"""
    c = run_length(n)
    return sorted({m // c for m in members})


def event_log_capacity(n):
    """include/swimsim.h, swimsim_applied_events: the per-Update log holds the larger of 4,096 and 4 x N rounded up to a
    multiple of 64 changes since the last drain"""
    return max(4096, 4 * padded(n))


# ---- A1: join lists ----
JOIN_SIZES = (1025, 1100, 2100, 3073)
JOIN_RUN_LENGTHS = {1025: 2, 1100: 2, 2100: 3, 3073: 4}
JOIN_FIRST_E = 20                                # call i carries incarnation t0 + (20 + i) periods


def join_observer(n):
    return n // 2


def join_lists(n):
    """[(members, incarnation)] of the four AddJoinList calls on join_observer(n): all alive, no source"""
    o = join_observer(n)
    others = [m for m in range(n) if m != o]
    sets = [others, sorted(random.Random(1).sample(others, int(0.4 * n))), [0, n - 1], [n - 1]]
    return [(ms, T0_MS + (JOIN_FIRST_E + i) * PERIOD_MS) for i, ms in enumerate(sets)]


def apply_join_list(sim, o, members, inc):
    """one call on an engine or an OracleSim; returns the applied count"""
    return sim.add_join_list(o, list(members), [ALIVE] * len(members), [inc] * len(members))


# ---- A2: protocol rounds ----
ROUNDS_SIZES = (1100, 2100)
ROUNDS_STEPS = (1,) * 8 + (4,)                   # 12 rounds: eight calls of one round, one of four
ROUNDS_BURST = 0.3


def rounds_observers(n):
    return (0, n // 2, n - 1)


def rounds_events(n):
    """int(0.3 N) members reincarnate in round 1 (a burst in round 0 would change nothing: the clock still reads t0)"""
    return [(1, EV_REINCARNATE, m, 0) for m in W.distinct_members(13, 1, 6, int(ROUNDS_BURST * n), n)]


def calls(steps, events):
    """[(first round, rounds, the events of those rounds)] of a step plan"""
    out, r = [], 0
    for k in steps:
        out.append((r, k, [e for e in events if r <= e[0] < r + k]))
        r += k
    return out


# ---- A3: fuzz schedules past one member per thread (a list of their own: fuzz_scenarios.CASES stays as committed) ----
FUZZ_N = 1100
FUZZ_SELF_SEED = 6                            # the smallest seed whose start is "self" (asserted on the host)
FUZZ_CASES = [(FUZZ_N, 0), (FUZZ_N, FUZZ_SELF_SEED)]


# ---- B: slots ----
SLOTS_N = 130
SLOTS_LOAD = dict(n=SLOTS_N, rounds=30, churn=0.05)
SLOTS_WATCHED = tuple(range(WATCH_SLOTS))        # observer o takes slot o
SLOTS_EXTRA = 64                                 # the 65th
SLOTS_UNDRAINED = (5, 63)                        # left undrained in rounds 0-9
SLOTS_GIVEN_UP, SLOTS_REUSER = 5, 100            # 5 is unwatched with changes logged; 100 takes its slot
SLOTS_SWITCHER = 7                               # "events" -> coalesced only -> "events"
SLOTS_REARMED = 9                                # watch(o, "events") again on an observer that already is "events"


def slots_mode(o):
    """even observers: the coalesced drain only; odd ones (63 in slot 63 among them): the per-Update stream too"""
    return "events" if o % 2 else True


def slots_workload():
    return W.config2(**SLOTS_LOAD)


# ---- C: overflow of the per-Update log ----
OVERFLOW_N = 64
OVERFLOW_WATCHED = (0, 1)
OVERFLOW_MEMBERS = list(range(1, OVERFLOW_N))    # 63 changes per call
OVERFLOW_FILL_CALLS = 65                         # 65 x 63 = 4,095 changes
OVERFLOW_ROUNDS = 116                            # the multi-round variant: every other member reincarnates each round


def overflow_call(sim, i):
    """call i = 1, 2, ...: observer 0 learns members 1..63 alive at t0 + i periods; returns the applied count"""
    return apply_join_list(sim, 0, OVERFLOW_MEMBERS, T0_MS + i * PERIOD_MS)


def overflow_events(rounds=OVERFLOW_ROUNDS):
    """members 1..63 reincarnate in each of the rounds 1..rounds-1"""
    return [(r, EV_REINCARNATE, m, 0) for r in range(1, rounds) for m in OVERFLOW_MEMBERS]


# ---- D: short caller buffers ----
SHORT_N = 130
SHORT_OBSERVER = 17
SHORT_WINDOW = 4                                 # churn rounds before each drain
SHORT_GUARD = 8                                  # sentinel entries behind cap
# what each window's two drains are called with: a cap (a number, or relative to the oracle's count k), every output
# array NULL with only the counts asked for, only the checksums asked for
SHORT_WINDOWS = (("cap", 0), ("cap", 1), ("cap", "k-1"), ("cap", "k"), ("counts", None), ("checksums", None))


def short_workload():
    return W.config2(n=SHORT_N, rounds=SHORT_WINDOW * len(SHORT_WINDOWS), churn=0.05)


def short_cap(spec, k):
    return {"k-1": k - 1, "k": k}.get(spec, spec)
