"""Scenarios that fill the message pool's sub-pools (tests/test_pool_host.py on the CPU oracle alone, tests/test_pool.py
engine against oracle). TEST INFRASTRUCTURE ONLY: pure Python, no GPU, no oracle import.

The pool (pool_alloc_lane0) is 64 sub-pools of pool records / 64 each; swimsim_create refuses a pool
below 64 x N records, so with an explicit message_pool_bytes the smallest sub-pool holds N records, against 16,384 and
more of the automatic pool. The pool is reset once per round and holds the round's requests and responses (and the
early response reservations, which may be twice the response). What a round asks of it is known from the oracle before
the engine runs: every live sender with a ping target issues its whole dissemination buffer, so the records of the
round's requests are the sum of the buffers' entry counts at the round's start (requests()).

SELFSTART  a self-only start with two seeds, seeded as tests/test_inbox_build.py seeds it. The buffers grow until a
           round's requests alone exceed a minimum pool (N = 512, by round 7); at N = 128 they never do, and a ladder of
           pools (minimum x 1, 2, 4, 16) runs the same rounds from tight to roomy.
HEAVY      a converged cluster of 256 whose first four observers each learn 200 newer incarnations by MakeChange. A
           message of more than sub / 2 = 128 records owns its sub-pool whichever sub-pool its wave started at, and
           more than 64 such allocations cannot fit in 64 sub-pools: overflow by counting. Left alone, the rows holding
           that many entries grow 4, 14, 59, 158 per round (a heavy row infects its target and, by its responses, the
           rows that ping it), which leaves one round between "a few" and "too many". So members 0..27 are partitioned
           off for rounds 0-4: the heavy rows stay among them (4, 10, 18, 22, 24, 27 at the starts of rounds 0-5, with
           ping-reqs and suspect declarations towards the unreachable majority beside them), and once the partition
           is lifted in round 5 they are 87 at the start of round 6.
SMALL      a self-only start with one seed at N = 512: 511 members ping member 0 with one record each. Its receive wave
           reserves one record per message (an allocation of at most sub / 256 = 2 records takes the fetch-add path),
           all from the sub-pool its wave starts at, which the requests of the senders 64, 128, ... share: 518 records
           asked of a sub-pool of 512, so a fetch-add cursor passes its sub-pool's end and the wave moves on.

An engine (swimsim.Cluster / ShardedCluster) and an OracleSim take the same calls.
"""
ALIVE = 0
T0_MS = 1_500_000_000_000
PERIOD_MS = 200
POOL_SUBS = 64                                   # POOL_SHARDS of swimsim_device.h
RECORD_BYTES = 16

SELFSTART = dict(n=128, seeds=2, rounds=16, ladder=(1, 2, 4, 16))
SELFSTART_FAIL = dict(n=512, seeds=2, rounds=8)  # round 7's requests alone exceed the minimum pool
SELFSTART_SHARDS = (2, 3)
EV_PARTITION = 5
HEAVY = dict(n=256, observers=(0, 1, 2, 3), members=range(40, 240), step=1, group=28, lift=5, rounds=7)
HEAVY["events"] = ([(0, EV_PARTITION, m, 1) for m in range(HEAVY["group"])] +
                   [(HEAVY["lift"], EV_PARTITION, m, 0) for m in range(HEAVY["group"])])
HEAVY_RECORDS = 128                              # sub / 2 at HEAVY's minimum pool: longer messages own a sub-pool
SMALL = dict(n=512, seeds=1, rounds=4)


def min_pool_records(n):
    """the smallest pool swimsim_create accepts: every sub-pool holds the longest message, N records"""
    return POOL_SUBS * n


def pool_records(n, mult=1):
    """the minimum pool times `mult` (a rung; may be a fraction such as 1.5), whole records per sub-pool"""
    return int(n * mult) * POOL_SUBS


def pool_bytes(n, mult=1):
    return pool_records(n, mult) * RECORD_BYTES


def seed_selfstart(n, seeds, *sims):
    """every node learns members 0..seeds-1 by MakeChange before round 0 (tests/test_inbox_build.py seed())"""
    for o in range(n):
        for m in range(seeds):
            if m != o:
                for s in sims:
                    s.make_change(o, m, T0_MS, ALIVE)


def seed_heavy(*sims):
    """HEAVY's observers each apply 200 changes: members 40..239 alive one period newer than the converged start"""
    for o in HEAVY["observers"]:
        for m in HEAVY["members"]:
            got = [s.make_change(o, m, T0_MS + HEAVY["step"] * PERIOD_MS, ALIVE) for s in sims]
            assert all(g == 1 for g in got), (o, m, got)


def requests(ora):
    """records of the coming round's requests: the buffers of the live senders (every node is live here, and every
    node of these scenarios knows a pingable member)"""
    return sum(ora.changes_count(o) for o in range(ora.n))


def heavy_rows(ora, above):
    """rows whose dissemination buffer holds more than `above` entries"""
    return sum(ora.changes_count(o) > above for o in range(ora.n))
