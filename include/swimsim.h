/*
 * swimsim.h — C ABI of libswimsim.so, the MI355X-native SWIM protocol-round engine.
 *
 * This is the drop-in boundary for ringpop-go's swim hot path. The reference has no FFI: its
 * path sits behind the Go interface swim.NodeInterface (swim/node.go:137-147) and the internal
 * Memberlist / Disseminator / stateTransitions types. Each entry point below says which
 * reference call it replaces. INTEGRATION.md shows the cgo binding a maintainer would add.
 *
 * Conventions
 *  - One handle = one simulated cluster of N members. Observer o is member o's swim.Node.
 *  - Incarnations cross the ABI as int64 milliseconds, like swim.Member.Incarnation
 *    (member.go:52). Inside they are kept as e = (inc - t0_ms) / protocol_period_ms.
 *  - Status codes equal statePrecedence (member.go:112-128): alive 0, suspect 1, faulty 2,
 *    leave 3, tombstone 4. SWIMSIM_UNKNOWN (7) means "not in this node's memberlist".
 *  - Return values: 0 = OK, negative = SWIMSIM_E*. swimsim_last_error() gives the message.
 *    HIP errors are mapped, never aborted on. A failed swimsim_create / swimsim_group_create
 *    leaves no handle: swimsim_last_error(NULL) gives its message, on the thread that called it.
 *  - Calls on one handle must be serialized. swimsim_step() blocks and is deterministic.
 *  - The caller owns every output buffer (caller allocates, library fills). No device pointer
 *    escapes.
 */
#ifndef SWIMSIM_H
#define SWIMSIM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWIMSIM_ABI_VERSION 17   /* 17: swimsim_tuning.slot_bump and the unit "bump_by_slot" (results unchanged).
                                    16: swimsim_forward, swimsim_forward_census and swimsim_forward_times (read-only; the
                                    results of every earlier call unchanged).
                                    15: swimsim_ring_checksums, swimsim_ring_census and swimsim_ring_times (read-only; the
                                    results of every earlier call unchanged).
                                    14: swimsim_tuning.resp_echo and the unit "resp_echoed" (results unchanged).
                                    13: swimsim_pool_usage (a read-back; nothing else changed since 12). 12: the
                                    checksum block-stream dump call is gone (only a diagnostics build ever
                                    implemented it, and that build is gone); nothing else changed since 11 */

enum {
    SWIMSIM_OK = 0,
    SWIMSIM_EINVAL = -1,     /* bad argument */
    SWIMSIM_ENOMEM = -2,     /* device allocation failed */
    SWIMSIM_EHIP = -3,       /* HIP runtime error */
    SWIMSIM_ECAPACITY = -4,  /* a device pool overflowed (message / dense-snapshot pool) */
    SWIMSIM_ERANGE = -5      /* incarnation not representable as t0 + e*period; clock offset out of range */
};

enum { SWIMSIM_ALIVE = 0, SWIMSIM_SUSPECT = 1, SWIMSIM_FAULTY = 2, SWIMSIM_LEAVE = 3, SWIMSIM_TOMBSTONE = 4,
       SWIMSIM_UNKNOWN = 7 };
#define SWIMSIM_SOURCE_NONE (-1)

/* Mirrors swim.Options (swim/node.go:45-100) plus the simulation inputs. A zero field means
 * the reference default (util.SelectInt / SelectDuration semantics, util/util.go:220-245). */
typedef struct swimsim_config {
    uint32_t num_members;              /* N */
    uint32_t device;                   /* HIP device ordinal */
    int64_t t0_ms;                     /* clock at round 0 = initial incarnation (default 1.5e12) */
    uint32_t protocol_period_ms;       /* MinProtocolPeriod, default 200 (node.go:80) */
    uint32_t suspect_timeout_ms;       /* StateTimeouts.Suspect, default 5 s (node.go:75) */
    uint32_t faulty_timeout_ms;        /* StateTimeouts.Faulty, default 24 h (node.go:76) */
    uint32_t tombstone_timeout_ms;     /* StateTimeouts.Tombstone, default 1 min (node.go:77) */
    uint32_t ping_request_size;        /* PingRequestSize, default 3 (node.go:86). At most 8; more: SWIMSIM_EINVAL */
    uint32_t max_reverse_full_sync_jobs; /* MaxReverseFullSyncJobs, default 5 (node.go:96) */
    uint32_t p_factor;                 /* disseminator pFactor, default 15 (disseminator.go:35). The piggyback
                                          counter has 8 bits: p_factor * digits10(max(N - 1, 1)), the largest
                                          maxP of the handle, must be at most 255, else SWIMSIM_EINVAL */
    uint64_t seed;                     /* Philox key (docs/ROUND_SEMANTICS.md §6) */
    const char *addresses;             /* NULL: synthetic "10.%03u.%03u.%03u:7000"; else N fixed-width,
                                          strictly ascending addresses, each addr_stride bytes (shorter ones
                                          NUL-padded). Widths of 13..20 bytes; any other width, unequal
                                          widths or an address not above its predecessor: SWIMSIM_EINVAL. A
                                          record tail status + decimal(t0 + e * period) + ';' of more than
                                          24 bytes is refused the same way */
    uint32_t addr_stride;
    uint32_t max_rounds;               /* incarnation table capacity (default 65536 rounds) */
    uint64_t message_pool_bytes;       /* change-record pool; 0 = automatic */
    uint32_t observer_begin, observer_end; /* shard of observer rows held by this handle; 0,0 = all */
    const struct swimsim_tuning *tuning;   /* NULL: the production engine; else variants for tests (below). Callers
                                              zero-initialise the struct (memset), so a field added later reads 0 */
} swimsim_config;

/* Engine variants the tests and diagnostics select per handle (results are identical in every variant; only where
 * and how the work runs changes). Every field: -1 = the production default. */
typedef struct swimsim_tuning {
    int32_t hot_slots;        /* hot-column slots per row; 0 = no hot columns; default 2,048 */
    int32_t dense_slots;      /* dense snapshot slots (at least 64); default: 2 per row + 64, bounded by a third of
                                 the free HBM; small pools exercise the lazy-snapshot fallbacks */
    int32_t cs_async;         /* 0: every phase-C checksum on the main stream; default 1 (side stream) */
    int32_t cs_async_rows;    /* phase-C launches of at most this many rows go to the side stream; default 12,288 */
    int32_t cs_narrow_rows;   /* launches of at most this many rows use the narrow checksum kernel; 0 = the wide
                                 kernel only; default 8,192 */
    int32_t cs_ref;           /* the reference-row checksum path: 0 off, 1 wide launches (default), 2
                                 every launch of at least 1,024 rows */
    int32_t fault_inject;     /* tests only, bits: 1 = the reference-row path's buffers fail to allocate (the production
                                 kernels stay in charge, create and step succeed); 2 = the next reference-row launch fails
                                 with SWIMSIM_EHIP (the step returns it); 4 = exception rings of 8 entries (ring waits,
                                 wrap-arounds and the fallback rows run); 8 = dedup keys narrowed to 3 bits (fingerprint
                                 groups of unequal rows); 16 = the reference-row kernel's stager waves at raised issue
                                 priority (a schedule in which the chain waves drift apart); 32 = the reference-row
                                 path's exception entries capped at 24 per row (rows ending within the stager's
                                 prefetch of the cap); 64 = seeded sleeps before the reference-row kernel's hand-over
                                 waits and signals, bits 8-11 selecting the delayed roles (g/f chains, h chains,
                                 record stagers, window stagers), bits 12-30 the seed; 128 = no side-stream buffer
                                 set for the reference-row path (side launches keep the narrow kernel); 256 = side
                                 launches of 1,024 rows and more take that path (4,097 by default); 1024 = one
                                 generation of side-stream snapshot slots (phase C waits for the previous round's side
                                 launch); default 0. Results are identical with 4, 8, 16, 32, 64, 128, 256 and 1024. */
    int32_t defer_test;       /* tests only (ABI 6): which ways a deferred full-sync decision may be settled without a hash
                                 (DESIGN.md §5), bits: 1 = a still-clean sender's current row is not compared directly;
                                 2 = no checksum representatives; 4 = no undo log; 8 = the undo log holds 2 entries per
                                 row instead of 1,024 (a pending-live sender's receive wave then rebuilds its issue-time
                                 row once it has logged more); 16 = the representative table has one slot (every checksum
                                 collides, the last store wins, the losing decisions fall through). Results are
                                 identical with every combination; <= 0 (default, and the 0 an older caller's
                                 zero-initialised struct reads): the production engine */
    int32_t cs_defer;         /* lazy phase C (ABI 11): may a round inside a multi-round swimsim_step leave
                                 its dirty rows unhashed for a later round of the same call? -1 or 1 (default): yes, when
                                 a round follows in the call, the launch would stay on the main stream (more dirty rows
                                 than cs_async_rows), at least 3/4 of the dirty rows changed in this round and the
                                 round deferred at most NL/64 full-sync decisions; 0 (also what an older caller's
                                 zero-initialised struct reads): every round hashes its dirty rows, as before ABI 11;
                                 2 = tests only: whenever a round follows in the call. Every read-back and every
                                 decision that needs a checksum still gets it; results are identical in every mode */
    int32_t resp_echo;        /* echoed response records (ABI 14): may a ping or ping-req response leave out
                                 a record that only repeats what the sender's message has just told the receiver (same
                                 member, status and incarnation; never a tombstone record, never the sender's own
                                 member)? Such a record cannot apply at the sender. -1 or 1 (default, also with a NULL
                                 tuning block): yes; the entry is still counted, bumped and deleted as before, only its
                                 record is not written. 0 (also what an older caller's zero-initialised struct reads):
                                 every kept record is written, as before ABI 14. Results are identical either way */
    int32_t slot_bump;        /* bump by slot (ABI 17): may a sender whose message was a walk of its hot slots
                                 bump its piggyback counters from a bitmap of the slots it sent (one bit per slot, written
                                 at issue) instead of reading its records back from the pool? -1 or 1 (default, also with
                                 a NULL tuning block): yes; every other message is bumped from its records. 0 (also what
                                 an older caller's zero-initialised struct reads): every bump reads the records, as before
                                 ABI 17, and no bitmap is allocated. Results are identical either way */
} swimsim_tuning;
/* Environment, read at swimsim_create (A/B experiments; results are identical either way): SWIMSIM_SYNC_SPIN=0 waits for
 * the main stream's host round trips in the runtime's stream wait instead of polling an event; SWIMSIM_SIDE2=0 runs both
 * generations of side-stream checksum launches on one stream; SWIMSIM_CS_DEFER=0|1|2 overrides
 * swimsim_tuning.cs_defer; SWIMSIM_RESP_ECHO=0|1 overrides swimsim_tuning.resp_echo;
 * SWIMSIM_SLOT_BUMP=0|1 overrides swimsim_tuning.slot_bump; SWIMSIM_CS_DEFER_LOG=1 writes one stderr line per phase C that had a round to leave its rows
 * to (round, dirty rows, rows written in the round, deferred decisions, carried or hashed). */

/* Events applied in phase E of a round (docs/ROUND_SEMANTICS.md §4). */
enum {
    SWIMSIM_EV_KILL = 1,        /* process stops (unreachable, frozen) */
    SWIMSIM_EV_REVIVE = 2,      /* process back + Reincarnate (handlers.go:140-143) */
    SWIMSIM_EV_REINCARNATE = 3, /* memberlist.Reincarnate (memberlist.go:234-236) */
    SWIMSIM_EV_LEAVE = 4,       /* adminLeaveHandler (handlers.go:145-148) */
    SWIMSIM_EV_PARTITION = 5,   /* set partition label of member a to b */
    SWIMSIM_EV_HEAL = 6,        /* discoverProviderHealer.Heal on observer a (heal_via_discover_provider.go:120) */
    SWIMSIM_EV_REAP = 7,        /* reapFaultyMembersHandler on observer a (handlers.go:154-163) */
    SWIMSIM_EV_CLOCK = 8        /* observer a's clock offset becomes b periods (swimsim_set_clock_offset inside a
                                   multi-round step; ABI 7). In list order: a later reincarnate, revive or leave of a in
                                   the same round runs on the new clock. swimsim_step checks the clock events of its
                                   rounds before it runs any (SWIMSIM_ERANGE, SWIMSIM_EINVAL; no round advanced) */
};
typedef struct swimsim_event { uint32_t round; uint32_t kind; int32_t a; int32_t b; } swimsim_event;

enum {
    SWIMSIM_C_ROUNDS, SWIMSIM_C_PINGS, SWIMSIM_C_PINGS_OK, SWIMSIM_C_PINGREQS, SWIMSIM_C_HELPER_CALLS,
    SWIMSIM_C_HELPER_ERRORS, SWIMSIM_C_INCONCLUSIVE, SWIMSIM_C_SUSPECT_DECL, SWIMSIM_C_APPLIED,
    SWIMSIM_C_REFUTES, SWIMSIM_C_FULL_SYNCS, SWIMSIM_C_FULL_SYNCS_PINGREQ, SWIMSIM_C_RFS_DONE,
    SWIMSIM_C_RFS_OMITTED, SWIMSIM_C_TIMERS_FIRED, SWIMSIM_C_MSG_CHANGES, SWIMSIM_C_HEAL_ATTEMPTS,
    SWIMSIM_C_HEAL_FAILURES, SWIMSIM_NCOUNTERS
};

typedef struct swimsim swimsim_t;

/* ---- lifecycle: swim.NewNode (node.go:194-238) for every member, Destroy (node.go:306-318) ---- */
int swimsim_create(const swimsim_config *cfg, swimsim_t **out);
int swimsim_destroy(swimsim_t *h);
const char *swimsim_last_error(swimsim_t *h);
int swimsim_abi_version(void);

/* ---- initial state ---- */
/* converged bootstrap: bootstrapNodes + waitForConvergence + ClearChanges (heal_partition_test.go:416-422) */
int swimsim_init_converged(swimsim_t *h);
/* every node knows only itself (NewNode + MakeAlive(self)), maxP = pFactor (disseminator.go:62) */
int swimsim_init_self_only(swimsim_t *h);
/* raw row write, no side effects (scenario setup) */
int swimsim_set_member(swimsim_t *h, uint32_t observer, uint32_t member, int32_t status, int64_t inc_ms);
/* raw write of a whole row (status[N], inc_ms[N]; SWIMSIM_UNKNOWN = not a member), no side effects:
 * seeds an observer from a received membership, e.g. a joinResponse's (join_handler.go:27-32,
 * memberlist.go:325-334 takes unseen members wholesale). Incarnations must be t0 + e*period. */
int swimsim_set_row(swimsim_t *h, uint32_t observer, const uint8_t *status, const int64_t *inc_ms);
/* memberlist.MakeChange (memberlist.go:282-307): returns #applied (0/1) or an error */
int swimsim_make_change(swimsim_t *h, uint32_t observer, uint32_t member, int64_t inc_ms, int32_t status);
/* disseminator.ClearChanges (disseminator.go:217-221) */
int swimsim_clear_changes(swimsim_t *h, uint32_t observer);
/* memberlist.AddJoinList (memberlist.go:398-406), called by the joiner for each joinResponse
 * (join_sender.go:411): Update of the n changes (distinct members, as MembershipAsChanges lists them;
 * source -1 = not a member, source/source_inc_ms may be NULL), then ClearChange of every applied change
 * except the observer's own. One device launch. *applied = number of applied changes. */
int swimsim_add_join_list(swimsim_t *h, uint32_t observer, const int32_t *member, const int32_t *status,
                          const int64_t *inc_ms, const int32_t *source, const int64_t *source_inc_ms, size_t n,
                          uint32_t *applied);
int swimsim_set_live(swimsim_t *h, uint32_t member, int32_t live);
int swimsim_set_partition(swimsim_t *h, uint32_t member, int32_t label);
/* SWIMSIM_ERANGE when a clock offset in force (below) would put a node's clock before t0 at that round */
int swimsim_set_round(swimsim_t *h, uint32_t round);

/* ---- per-node clocks (ABI 7): swim.Options.Clock (node.go:45-100, 194-238), one clock per swim.Node ----
 * Observer o's clock in round r is now(o) = t0 + (r + k_o) * period; k_o (signed, whole periods, 0 at create) is
 * its offset: a skewed or stepped clock, as the reference's partition-heal tests give their two partitions
 * (heal_partition_test.go:447-454). The clock enters where the reference reads it: a refute's and Reincarnate's
 * incarnation (memberlist.go:337-354, 234-236) and the timer deadlines (state_transitions.go:119-160). Incarnations
 * and deadlines are absolute values in the owner's clock, so a change of k_o rewrites nothing: after a forward step
 * every timer with deadline <= now(o) fires in the next phase T, in (deadline, member) order, each with now =
 * deadline; after a backward step timers wait longer, and a refute or Reincarnate may write an incarnation below the
 * one held before (the node then loses to the rumour it refutes until its clock passes it). With every offset 0
 * results are bit-identical to a handle that never set one. Random streams, iterator epochs and counters stay on
 * the round.
 * Errors, before any state changes: SWIMSIM_EINVAL (NULL handle or pointer, observer >= N); SWIMSIM_ERANGE when
 * offset_ms is not a multiple of the period (the engine stores e), when |offset| > 32,767 periods (one step stays
 * below the lateness field of the per-Update stream's timer tags), or when round + k_o < 0 (a clock before t0).
 * Shards: like swimsim_set_live, every shard of a cluster takes the same calls and keeps the whole table. */
int swimsim_set_clock_offset(swimsim_t *h, uint32_t observer, int64_t offset_ms);
/* every offset with one upload: offset_ms[N] */
int swimsim_set_clock_offsets(swimsim_t *h, const int64_t *offset_ms);
/* the offsets in force, in ms: out[N] */
int swimsim_clock_offsets(swimsim_t *h, int64_t *out);

/* ---- the hot path: nrounds protocol periods of every live node (gossip.ProtocolPeriod,
 *      gossip.go:178-188, for all N nodes under docs/ROUND_SEMANTICS.md). events are applied
 *      in phase E of the round equal to their .round field.
 *      SWIMSIM_ECAPACITY (a device pool overflowed: swimsim_last_error names it) is detected once, after the last
 *      round of the call: the round whose allocation failed went on with empty messages in place of the ones that
 *      did not fit, and the call's later rounds ran on top of it. The handle's protocol state is then unspecified
 *      (no read-back of it is meaningful, and swimsim_round counts every round of the call); every access stayed
 *      inside the handle's buffers, the error word is cleared, and the process and its other handles are unaffected.
 *      Destroy the handle and create one with larger pools (swimsim_config.message_pool_bytes). A caller that must
 *      know the last good round steps one round per call. The same holds for swimsim_heal and swimsim_group_step. ---- */
int swimsim_step(swimsim_t *h, uint32_t nrounds, const swimsim_event *events, size_t nevents);
/* Heal() on one observer right now (heal_via_discover_provider.go:120-177); targets may be NULL */
int swimsim_heal(swimsim_t *h, uint32_t observer, int32_t *targets, size_t cap, size_t *ntargets);

/* ---- read-back: NodeInterface / memberlist / disseminator views ---- */
uint32_t swimsim_round(swimsim_t *h);
/* GetChecksum (node.go:137-147 → memberlist.Checksum, memberlist.go:73-80), all observers */
int swimsim_checksums(swimsim_t *h, uint32_t *out);
/* memberlist.GetMembers (memberlist.go:459-468) as a dense row: status[N], inc_ms[N] */
int swimsim_row(swimsim_t *h, uint32_t observer, uint8_t *status, int64_t *inc_ms);
/* CountReachableMembers (memberlist.go:485-497) */
int swimsim_count_reachable(swimsim_t *h, uint32_t observer, uint32_t *out);
/* GetReachableMembers (memberlist.go:471-483): member indices, ascending */
int swimsim_reachable(swimsim_t *h, uint32_t observer, uint32_t *idx, size_t cap, size_t *n);
/* NumPingableMembers (memberlist.go:188-198), disseminator.maxP (disseminator.go:49),
 * ChangesCount (disseminator.go:239-244), NumMembers (memberlist.go:174-179) */
int swimsim_node_stats(swimsim_t *h, uint32_t observer, int32_t *pingable, int32_t *maxp,
                       int32_t *changes, int32_t *members);
/* disseminator.changes: members, p, source (or -1), source incarnation (ms) */
int swimsim_changes(swimsim_t *h, uint32_t observer, int32_t *member, int32_t *p, int32_t *source,
                    int64_t *source_inc_ms, size_t cap, size_t *n);
/* stateTransitions.timers: members, state, fired, deadline (ms), subject incarnation (ms) */
int swimsim_timers(swimsim_t *h, uint32_t observer, int32_t *member, int32_t *state, int32_t *fired,
                   int64_t *deadline_ms, int64_t *subject_inc_ms, size_t cap, size_t *n);
/* memberlistIter state: currentIndex, number of reshuffles */
int swimsim_iter_state(swimsim_t *h, uint32_t observer, int64_t *idx, uint32_t *epoch);
/* phase-S ping targets of the last round (-1 = none) */
int swimsim_last_targets(swimsim_t *h, int32_t *out);
int swimsim_counters(swimsim_t *h, uint64_t *out);
/* canonical state digests (same definition as the oracle): rows, dissemination, timers */
int swimsim_digest(swimsim_t *h, uint64_t *rows, uint64_t *dissemination, uint64_t *timers);
/* converged (test_utils.go:188-198): no live node has changes and all live checksums equal */
int swimsim_converged(swimsim_t *h, int32_t *out);

/* ---- upward coupling: NodeInterface.RegisterListener (node.go:146) ----
 * MemberlistChangesAppliedEvent{Changes, OldChecksum, NewChecksum, NumMembers} (swim/events.go:56-61) is
 * emitted by memberlist.Update whenever it applied something (memberlist.go:366-384); Ringpop feeds its
 * hash ring from it (ringpop.go:398-400,550-563). Watch an observer to record its applied changes (off by
 * default: unwatched rows pay one predicated branch per applied change); a drain returns, in member order,
 * the last applied change of every member since the previous drain (the per-Update events of the rounds in
 * between, coalesced per member: the ring's final membership depends only on each member's last change),
 * the checksum at the previous drain (OldChecksum), the current one (NewChecksum) and NumMembers. n = 0:
 * nothing applied, no event. Evictions are not events (RemoveMember emits none, memberlist.go:141-162).
 * At most 64 watched observers per handle.
 * on = 1: the coalesced drain below. on = 2: also the per-Update stream (swimsim_applied_events). on = 0: off (the
 * observer's slot is free again and what its logs still held is dropped). Any other value of on is refused with
 * SWIMSIM_EINVAL before anything is allocated or changed. */
int swimsim_watch(swimsim_t *h, uint32_t observer, int32_t on);
int swimsim_applied_changes(swimsim_t *h, uint32_t observer, int32_t *member, int32_t *status, int64_t *inc_ms,
                            int32_t *source, int64_t *source_inc_ms, size_t cap, size_t *n, uint32_t *old_checksum,
                            uint32_t *new_checksum, int32_t *num_members);
/* The per-Update stream of an observer watched with on = 2, without coalescing: one event per Update that applied
 * something (memberlist.go:366-384), in the order the node ran its Updates (docs/ROUND_SEMANTICS.md §4: events, each
 * fired timer in (deadline, member) order, the inbox in sender order, the response, the ping-req relays, the
 * reverse full syncs). Change i belongs to event event[i] (0 .. *nevents-1, ascending); the changes of one event
 * are listed in member order (the reference lists a message's changes in Go map order, which is random). Ringpop's
 * per-change statistics (ringpop.go:398-406) and its ring's insertion order are those of this stream.
 * OldChecksum / NewChecksum / NumMembers are per DRAIN, not per event: the checksum at the previous drain of this
 * stream, the current checksum and the current member count (the reference computes one checksum per Update,
 * memberlist.go:367; this engine keeps the per-round ones). *n = total changes (also when > cap: only cap are
 * written). The log of one observer holds the larger of 4,096 and 4 x N' changes since its last drain, N' = N rounded
 * up to a multiple of 64 (4,096 changes up to N = 1,024). SWIMSIM_ECAPACITY: more changes than that were applied since
 * the last drain; nothing is written, the stream restarts empty and the next drain's OldChecksum is the checksum at
 * the refused one. The coalesced drain of the same observer is not affected. */
int swimsim_applied_events(swimsim_t *h, uint32_t observer, int32_t *member, int32_t *status, int64_t *inc_ms,
                           int32_t *source, int64_t *source_inc_ms, uint32_t *event, size_t cap, size_t *n,
                           size_t *nevents, uint32_t *old_checksum, uint32_t *new_checksum, int32_t *num_members);

/* NodeInterface.ProtocolStats (node.go:137-147, stats.go:81-104). Each round is one ProtocolPeriod of every
 * live node (gossip.go:178-188), so the Timing histogram is over rounds: the device wall time of each round
 * (HIP events on the engine's stream), in ns. ProtocolRate = max(2 x median, MinProtocolPeriod)
 * (AdjustProtocolRate, gossip.go:110-115). ServerRate = pings and ping-reqs handled per node per simulated
 * second (ping_handler.go:37, ping_request_handler.go:45); ClientRate is never marked by the reference (0).
 * Deviation (documented, not pinnable): the reference's Timing is metrics.NewHistogram(NewUniformSample(10))
 * (gossip.go:65), so its Min/Max/Sum/Mean/Variance/percentiles come from a 10-element random reservoir (Count is
 * the total), and AdjustProtocolRate takes that reservoir's median; its rates are go-metrics Meter.Rate1() (a
 * one-minute EWMA). Here every statistic is over every round (up to 2^20) and rates are means over the run. The
 * reservoir is filled from Go's global math/rand, so no restatement could match it sample for sample. */
typedef struct swimsim_protocol_stats {
    int64_t count;
    double min_ns, max_ns, sum_ns, mean_ns, variance, stddev_ns, median_ns, p75_ns, p95_ns, p99_ns, p999_ns;
    int64_t protocol_rate_ns;
    double client_rate, server_rate, total_rate;
} swimsim_protocol_stats_t;
int swimsim_protocol_stats(swimsim_t *h, swimsim_protocol_stats_t *out);

/* device memory of the handle (DESIGN.md §2 budget): bytes of the row words, dissemination entries (+ presence
 * bits), timers (+ block bounds), message pool and dense snapshots, total bytes held; the dense-snapshot slots
 * (main, side stream) and how many phases hashed their dirty senders before issue because the lazy C_o
 * snapshots would not have fit in the slots (exact either way) */
typedef struct swimsim_memory_t {
    uint64_t row_words, dissemination, timers, message_pool, dense_snapshots, total;
    uint32_t dense_cap, side_cap;
    uint64_t lazy_fallbacks;
} swimsim_memory_t;
int swimsim_memory(swimsim_t *h, swimsim_memory_t *out);
/* the message pool's fill (ABI 13; a copy of 64 words, no launch): the pool is 64 sub-pools of *sub_records change
 * records each, and cursors[s] is the number of records taken from sub-pool s since the cursors were last reset,
 * which is at the start of every round and of swimsim_heal: after swimsim_step(h, 1, ...) they describe that round,
 * early response reservations included. A cursor above *sub_records: an allocation of at most sub_records / 256
 * records did not fit there and moved on to the next sub-pool (the sub-pool is full). All 0 before the first round. */
int swimsim_pool_usage(swimsim_t *h, uint64_t *sub_records, uint64_t *cursors /* [64] */);

/* ---- member census (ABI 8): how the cluster sees each member ----
 * No reference counterpart: these stand in for polling NodeInterface.MemberStats (stats.go:41-52) on every node and
 * counting, per member, the states the nodes hold it in. A census is a read-only column reduction over the handle's
 * observer rows on the device: it changes no state and no result of the round.
 *
 * swimsim_census: counts[i*6 + s] = the number of counted observer rows of this handle that hold member members[i] in
 * status s: 0..4 = alive, suspect, faulty, leave, tombstone, 5 = unknown (the row word's SWIMSIM_UNKNOWN, evicted
 * members included). min_inc_ms[i] / max_inc_ms[i] (either may be NULL) = the smallest / largest incarnation over the
 * counted rows that know the member, both -1 when none does. who = SWIMSIM_CENSUS_LIVE counts the owned rows whose
 * observer is live now (the table swimsim_set_live and the kill / revive events write), SWIMSIM_CENSUS_ALL every owned
 * row; an observer's own cell counts like any other. members = NULL: every member in index order, and n must be N;
 * else n indices below N (duplicates allowed), and the read-back is proportional to n. ms (may be NULL) receives the
 * HIP-event time of the device work. One host synchronisation per call. SWIMSIM_EINVAL, before any device work: NULL
 * handle or counts, n = 0, an index >= N, NULL members with n != N, an unknown who.
 *
 * swimsim_trace_members: track n <= 64 members (more, or an index >= N: SWIMSIM_EINVAL) in a buffer of rounds_cap
 * (1..65,536) records allocated here (SWIMSIM_ENOMEM). While a trace is set every round of swimsim_step appends, with
 * one kernel after phase C and no host round trip, the record {round, live owned observers, counts[n][6] over the live
 * owned rows}; with rounds_cap records held, later rounds are dropped and counted. A new call replaces the set and
 * clears the records; n = 0 switches the trace off and frees it.
 *
 * swimsim_trace_read: drains the trace in round order: at most cap records are written (rounds[k], nlive[k],
 * counts[k*n*6 ...]; each may be NULL), *n = the records held, *dropped = the rounds lost since the last drain. The
 * trace is empty afterwards and keeps recording. No trace set: *n = 0.
 *
 * Shards: a handle counts its own rows, and every shard keeps the whole live table (swimsim_set_live). Counts add
 * across shards; incarnation minima and maxima combine across shards with -1 as the identity; nlive adds across shards,
 * and the shards' records line up by round. Census scratch and the trace buffer are allocated on first use: a handle
 * that never calls these keeps the swimsim_memory figures it had. */
enum { SWIMSIM_CENSUS_LIVE = 0, SWIMSIM_CENSUS_ALL = 1 };
int swimsim_census(swimsim_t *h, const uint32_t *members, size_t n, int32_t who, uint32_t *counts, int64_t *min_inc_ms,
                   int64_t *max_inc_ms, double *ms);
int swimsim_trace_members(swimsim_t *h, const uint32_t *members, size_t n, uint32_t rounds_cap);
int swimsim_trace_read(swimsim_t *h, uint32_t *rounds, uint32_t *nlive, uint32_t *counts, size_t cap, size_t *n,
                       uint32_t *dropped);

/* ---- key routing through every node's own ring view (ABI 9) ----
 * Every Ringpop node feeds its consistent-hash ring from its own memberlist: alive and suspect members are servers,
 * every other status is not (Ringpop.handleChanges, ringpop.go:550-563), and Lookup (ringpop.go:582-606) asks that
 * ring. These calls answer, on the device, where observer o sends key k, for every observer row of the handle, without
 * a ring per node. They are read-only: no state and no result of the round changes.
 *
 * The view ring of observer o with R replica points is the ring one AddRemoveServers builds on an empty
 * hashring.HashRing: it adds every member whose cell in row o is alive or suspect, in ascending member index, and
 * removes nothing. Its points are Fingerprint32(address(m) ‖ decimal(i)), i = 0..R-1; at an equal hash the lowest
 * present member index owns the point (first inserter keeps it, rbtree.go:122-126); owner(o, k) is the member index of
 * the first point >= Fingerprint32(key k) in (hash, member) order, wrapping to the first point; an empty ring gives -1.
 *
 * Deviation: a real node's ring depends on its history at a shared hash, because removing one server deletes the
 * point for both (hashring.go:182-188); the view ring is the fresh build. With the synthetic addresses, N = 256 and
 * R = 100, members 185 and 215 share replica hash 581480965 and "key-226936" (hash 581472960) is owned by 185 with
 * every member present, by 215 without 185, by 97 without both, and by 97 in a ring from which 185 was removed after
 * the build: the last is what a long-running node answers, 215 what the view ring answers.
 *
 * Keys are packed as for swimring_lookup_batch: key k is bytes [off[k], off[k+1]) of keys. mode: 0 = automatic, 1 =
 * the ring walk for every row, 2 = the direct path for every row whose servers fit its list of 512 (diagnostics: the
 * results are identical in every mode). replica_points is 1..1000 (with addresses of 13..20 bytes every replica string
 * is then 14..23 bytes, one FarmHash length path). ms (may be NULL) receives the HIP-event time of the device work
 * (without the point table, which is built at the first use of a replica_points value and kept).
 *
 * swimsim_route: owners[j*nkeys + k] = owner(observers[j], k). Observers must be rows of this handle; the read-back
 * is proportional to nobs * nkeys.
 *
 * swimsim_route_census: who = SWIMSIM_CENSUS_LIVE or SWIMSIM_CENSUS_ALL selects the counted rows as for swimsim_census;
 * *counted = their number. For key k, entries [hist_off[k], hist_off[k+1]) list every distinct owner over the counted
 * rows, ascending by owner (-1 first), each with the number of counted rows that answer it; zero counts are omitted
 * and the counts of one key sum to *counted. *nhist = the total number of entries; at most cap are written to
 * hist_owner / hist_count and the caller retries with larger buffers (no error); hist_off (nkeys + 1 entries) is always
 * complete. The device appends only the (key, owner) pairs that differ from the owner under the first counted row,
 * sorts them and counts the runs: the result does not depend on arrival order, and a cluster that agrees writes
 * nothing. One host synchronisation per pass over the rows when the views agree, one more to read the runs when they
 * do not; a pass whose pairs overflow the buffer is run again over fewer keys, never truncated.
 *
 * SWIMSIM_EINVAL, before any device work: NULL handle (-1, nothing written), keys, off or output; nkeys = 0;
 * replica_points outside 1..1000; an observer out of range or not owned; nobs = 0; an unknown who or mode; N above
 * 524,288 (the row's presence bitmap is then more than 64 KB of LDS). SWIMSIM_ENOMEM leaves the handle usable.
 *
 * Shards: a handle routes over its own rows; histograms add across shards per (key, owner). Memory: the point table
 * (12 bytes per member and replica point) and at most 256 MiB of scratch beyond it and the keys are allocated on first
 * use and freed at destroy: a handle that never calls these launches what it launched and keeps the swimsim_memory
 * figures it had. */
int swimsim_route(swimsim_t *h, const uint8_t *keys, const uint64_t *off, size_t nkeys, uint32_t replica_points,
                  const uint32_t *observers, size_t nobs, int32_t mode, int32_t *owners, double *ms);
int swimsim_route_census(swimsim_t *h, const uint8_t *keys, const uint64_t *off, size_t nkeys, uint32_t replica_points,
                         int32_t who, int32_t mode, uint32_t *counted, uint64_t *hist_off, int32_t *hist_owner,
                         uint32_t *hist_count, size_t cap, size_t *nhist, double *ms);

/* ---- replica sets through every node's own ring view (ABI 10) ----
 * Ringpop's second routing call, LookupN (ringpop.go:611, hashring.go:268-301), returns the n distinct servers that
 * hold a key; replica.Replicator fans reads and writes out over that set (replica/replicator.go:170-213, NValue 3).
 * These calls answer it through the view ring of every observer row (the ring of ABI 9 above: the fresh
 * AddRemoveServers build from the members row o holds alive or suspect; its deviation note applies unchanged). They are
 * read-only as the ABI 9 calls are. cnt(o) is the view's server count.
 *
 * prefs(o, k, n), 1 <= n <= 16:
 *   cnt(o) <= n   every server of the view in ascending member index, cnt(o) entries (hashring.go:280-282, the rule of
 *                 swimring_lookup_n_batch); an empty view gives 0 entries.
 *   otherwise     start at the first REAL point >= Fingerprint32(k) in (hash, member) order, wrap once, and list each
 *                 distinct owner at its first occurrence until n are listed.
 * A point is real only for the lowest present member at its hash: when present members a < b share a replica hash the
 * tree holds one node, a's (rbtree.go:122-126), and b's replica is not a point of this view: it must not add b to the
 * list. If a is absent, b's point is real. Lookup never sees this (a comes first in the walk); LookupN does: with the
 * synthetic addresses, N = 256, R = 100 and every member present, members 185 and 215 share replica hash 581480965 and
 * prefs(o, "key-226936", 3) = 185, 97, 55, not 185, 215, 97. The order is the walk's order, a stronger promise than the
 * reference's (which returns from a Go map) and the one swimring_lookup_n_batch makes.
 *
 * swimsim_route_n: prefs[(j*nkeys + k)*n + i], i < min(n, cnt(observers[j])), is the list; the rest of the n slots is
 * -1. servers[j] (may be NULL) = cnt(observers[j]). keys, off, replica_points, mode, ms and the rule that observers are
 * rows of this handle are those of swimsim_route; mode 2 takes the direct path for rows of n < cnt <= 512 servers.
 *
 * swimsim_replica_census: who, *counted, cap / *nhist (retry with larger buffers, no error) and the always-complete
 * hist_off are those of swimsim_route_census. For key k, entries [hist_off[k], hist_off[k+1]) list every member that is
 * in the replica set of k under at least one counted row, ascending by member, each with the number of counted rows
 * whose set holds it (the sets are unordered here). Zero counts are omitted, every count is <= *counted, and the counts
 * of one key sum to the sum over the counted rows of min(n, cnt(row)). All counted rows agree on key k's replica set
 * exactly when every listed member has count = *counted. The device appends, per row and key, only the members by
 * which the row's set differs from the set under the first counted row (a cluster that agrees writes nothing), sorts
 * them and counts the runs, as swimsim_route_census does; a pass that overflows the buffer is run again over fewer keys.
 *
 * SWIMSIM_EINVAL, before any device work and with nothing written: every case of the ABI 9 calls, and n = 0 or
 * n > 16. SWIMSIM_ENOMEM leaves the handle usable. Shards: as for ABI 9; histograms add per (key, member). Memory: on
 * first use, freed at destroy; beside the ABI 9 buffers (which these calls share, the point table included) nkeys * n
 * words for the base sets, and the census's pair buffers hold at least 2 * n * (rows of the handle) pairs of 28 bytes
 * (448 MiB for 524,288 rows and n = 16). A handle that never calls these launches what it launched and keeps the
 * swimsim_memory figures it had; swimsim_route and swimsim_route_census keep their kernels and results. */
int swimsim_route_n(swimsim_t *h, const uint8_t *keys, const uint64_t *off, size_t nkeys, uint32_t replica_points,
                    uint32_t n, const uint32_t *observers, size_t nobs, int32_t mode, int32_t *prefs, uint32_t *servers,
                    double *ms);
int swimsim_replica_census(swimsim_t *h, const uint8_t *keys, const uint64_t *off, size_t nkeys, uint32_t replica_points,
                           uint32_t n, int32_t who, int32_t mode, uint32_t *counted, uint64_t *hist_off,
                           int32_t *hist_member, uint32_t *hist_count, size_t cap, size_t *nhist, double *ms);

/* ---- ring checksums through every node's own ring view (ABI 15) ----
 * Ringpop.Checksum (ringpop.go:571-577) returns hashring.Checksum: Fingerprint32 of the ring's servers, sorted and
 * joined by ";" (hashring.go:100-107). A node publishes it as the ring.checksum gauge and the ring.checksum-periodic
 * stat (ringpop.go:209-217, 502-504) and in /admin/stats (stats_handler.go:56); two nodes with different ring checksums
 * route some keys differently. These calls answer it, on the device, for every observer row of the handle. They are
 * read-only as the ABI 8-10 calls are: no state and no result of a round changes.
 *
 * The servers of view o are the members whose cell in row o is alive or suspect: the set of ABI 9 and 10.
 * ringcs(o) = Fingerprint32(S), S = the servers' addresses in ascending member index joined by ";" with no trailing
 * separator. The addresses of a handle are fixed-width (W = 13..20 bytes) and strictly ascending, so sort.Strings order
 * is index order, and S has cnt * (W + 1) - 1 bytes for cnt servers: the empty string for an empty view (3696677242),
 * one address (13..20 bytes) for cnt = 1, at least 27 bytes otherwise. The synthetic addresses of members 0..4 give
 * 2141723838. This is not the membership checksum of swimsim_checksums: incarnations and the alive / suspect
 * distinction do not enter it.
 *
 * No deviation: Ringpop.handleChanges adds a server on alive and suspect and removes it on every other status
 * (ringpop.go:550-563), and the checksum is a function of the server SET alone, so a real node's value is exactly this
 * one whatever its history. The shared-hash history deviation of ABI 9 and 10 concerns replica points, which the
 * checksum does not read.
 *
 * swimsim_ring_checksums: checksums[j] = ringcs(observers[j]); servers[j] (may be NULL) = that view's server count.
 * observers must be rows of this handle; duplicates are allowed; observers = NULL means every owned row in order, and
 * nobs must then be the number of owned rows. The read-back is proportional to nobs.
 *
 * swimsim_ring_census: who = SWIMSIM_CENSUS_LIVE or SWIMSIM_CENSUS_ALL selects the counted rows as for swimsim_census;
 * *counted = their number. One entry per distinct checksum value over the counted rows, ascending by checksum:
 * hist_count = the counted rows that answer it, hist_first = the lowest global observer index among them, hist_servers
 * = that row's server count. Two different views with equal checksums form one entry, as the gauge would show. The
 * counts sum to *counted. *nhist = the number of entries; at most cap are written and the caller retries with larger
 * buffers (no error, as swimsim_route_census). No counted rows: *counted = 0 and *nhist = 0.
 *
 * mode: results are identical in every mode. 0 = production: rows whose views are equal share one FarmHash chain. Rows
 * are grouped by a 64-bit order-free key of the server set and the server count, every grouped row is then compared
 * with its group's lowest row member by member on the device, and a row that differs runs its own chain: a key
 * collision never gives a wrong checksum. 1 = every row runs its own chain. 2 = tests only: the grouping key is
 * narrowed to 3 bits, so that unequal views share a key and only the exact comparison parts them (the precedent is
 * fault_inject 8 on the membership path). *hashed (may be NULL) = the chains the call ran: the rows in mode 1; in mode
 * 0 the distinct views among the rows unless two views share the key, then more, never fewer. ms (may be NULL) = the
 * HIP-event time of the device work; swimsim_ring_times gives the last call's split over the scan, the exact
 * comparison and the chains with their scatter.
 *
 * At most three host synchronisations per call: the keys (12 bytes per row), the comparison's flags (4 bytes per row;
 * only when some group has more than one row) and the checksums. Memory: 36 bytes per requested row, allocated on
 * first use and freed at destroy: a handle that never calls these launches what it launched and keeps the
 * swimsim_memory figures it had.
 *
 * SWIMSIM_EINVAL, before any device work and with nothing written: NULL handle (-1) or NULL required output; nobs = 0;
 * NULL observers with nobs not the number of owned rows; an observer out of range or not owned; an unknown who or mode;
 * N above 524,288 (the bound of the route calls' LDS bitmap). SWIMSIM_ENOMEM leaves the handle usable.
 *
 * Shards: a handle answers for its own rows; histograms add per checksum across shards, hist_first is the minimum and
 * hist_servers follows it. */
int swimsim_ring_checksums(swimsim_t *h, const uint32_t *observers, size_t nobs, int32_t mode, uint32_t *checksums,
                           uint32_t *servers, uint32_t *hashed, double *ms);
int swimsim_ring_census(swimsim_t *h, int32_t who, int32_t mode, uint32_t *counted, uint32_t *hist_checksum,
                        uint32_t *hist_count, uint32_t *hist_servers, uint32_t *hist_first, size_t cap, size_t *nhist,
                        uint32_t *hashed, double *ms);
int swimsim_ring_times(swimsim_t *h, double *scan_ms, double *group_ms, double *hash_ms);

/* ---- requests forwarded through every node's own ring view (ABI 16) ----
 * A Ringpop node does not stop at Lookup. HandleOrForward (ringpop.go:687-712) handles a key itself when
 * Lookup(key) == WhoAmI() and otherwise calls the owner through forward.Forwarder.ForwardRequest
 * (forward/forwarder.go:156-174); that node runs HandleOrForward again, through its own ring. While the views disagree a
 * request can die at a node that is gone, take extra hops, bounce between a node that has left and the nodes that have
 * not heard yet, or be served by two nodes at once. These calls follow every request from node to node, on the device,
 * for the state after the last round. They are read-only as the ABI 8-15 calls are: no state and no result of a round
 * changes.
 *
 * owner(h, k) is the view-ring owner of ABI 9 (its deviation note applies unchanged);
 * reach(a, b) = live(a) and live(b) and part(a) == part(b), as in docs/ROUND_SEMANTICS.md. A request for key k enters at
 * node e with max_hops (1..64) forwards allowed:
 *
 *   if !live(e): ENTRY_DOWN, handler -1, hops 0
 *   h = e, hops = 0
 *   loop:
 *     d = owner(h, k)
 *     d == -1            -> NO_OWNER    (Lookup errs on an empty ring, ringpop.go:694-697)
 *     d == h             -> hops == 0 ? LOCAL : DELIVERED; handler = h
 *     hops == max_hops   -> HOP_LIMIT   (the request would need one forward more)
 *     !reach(h, d)       -> UNREACHABLE (the forward call errs; holder = h, next = d)
 *     h = d; hops += 1
 *     policy ONE_HOP     -> DELIVERED, handler = h   (the forwarded header: a forwarded call is never forwarded again,
 *                                                     forward/forwarder.go:176-201)
 *
 * Chains cannot loop while every holder holds itself alive or suspect: along a chain the clockwise distance from the
 * key to the chosen point strictly falls, in (hash, member) order. (Node h forwards to d because d's point p is the
 * first point >= the key among the servers of h's view. If d holds itself a server, p is a point of d's view too, so
 * d's own choice is p or a point before it; d forwards on only when that point is strictly nearer the key.) A chain
 * loops only through a node that is no server in its own ring, such as a node that has left and still runs.
 * HOP_LIMIT therefore reports either a chain longer than max_hops or such a bounce.
 *
 * Retries are outside these calls. The reference retries over wall-clock time: MaxRetries is 3, after 3, 6 and 12 s,
 * which is 15, 30 and 60 rounds at the default period, and AttemptRetry looks the key up again on each retry
 * (forward/request_sender.go:206-243). UNREACHABLE is the outcome of one attempt. A caller models retries by stepping
 * the cluster and asking again, with the holder as the entry node: that is why swimsim_forward takes arbitrary
 * (entry, key) pairs.
 *
 * keys, off and replica_points are those of swimsim_route. policy: SWIMSIM_FWD_CHAIN = HandleOrForward at every hop,
 * SWIMSIM_FWD_ONE_HOP = the first forward delivers.
 *
 * swimsim_forward: request i is key key_index[i] entering at node entry[i], nreq requests; duplicates are allowed.
 * key_index = NULL: entry lists nreq / nkeys entry nodes (nreq must be a multiple of nkeys) and request j*nkeys + k is
 * key k entering at entry[j]. outcome[i] and hops[i] (the forwards made) are required; handler[i] (the node that serves
 * the request, -1 when none does), holder[i] (the node where the chain ended: the handler, the node whose call failed,
 * the last holder, or the entry node) and next[i] (the destination that was not reached, for UNREACHABLE and HOP_LIMIT;
 * otherwise -1) may each be NULL. The read-back is proportional to nreq; one host synchronisation per call.
 *
 * swimsim_forward_census: the entries are all rows whose observer is live; *counted = their number.
 * outcomes[k*6 + c] counts the outcomes of key k and hops_hist[k*(max_hops+1) + j] the requests of key k that ended
 * after j forwards; both sum to *counted per key. For key k, entries [hist_off[k], hist_off[k+1]) list every distinct
 * handler, ascending, -1 first ("not served"), each with the number of entries whose request ends there; the counts of
 * one key sum to *counted. A key is split when it has more than one handler >= 0. cap, *nhist (retry with larger
 * buffers, no error) and the always-complete hist_off are those of swimsim_route_census, as are the pair buffers, the
 * sort and the run count: the device stages only the (key, handler) pairs that differ from the handler under the first
 * counted entry, so the result does not depend on arrival order and a cluster that agrees writes nothing; a pass whose
 * pairs overflow is run again over fewer keys, never truncated. Host synchronisations per pass as for
 * swimsim_route_census, and one more for the bins.
 *
 * mode: results are identical in every mode. 0 = production; 1 and 2 pass through to the route kernel's walk and direct
 * path; 3 = tests only: the owner table holds 8 keys per pass, so small tests run several passes and a last partial
 * one. ms (may be NULL) = the HIP-event time of the device work; swimsim_forward_times gives the last call's split
 * over the owner table, the chases and (census) the rest: the keys' hashes, the pair sort and the run count.
 *
 * SWIMSIM_EINVAL, before any device work and with nothing written: every case of swimsim_route (NULL handle: -1);
 * max_hops outside 1..64; an unknown policy or mode; an entry or key index out of range; nreq = 0, or no multiple of
 * nkeys with key_index = NULL; a NULL required output; a handle that does not own every row: a chain may visit any
 * row, and chains that cross shards are out of scope (the error text says so). SWIMSIM_ENOMEM leaves the handle usable.
 *
 * Memory, on first use and freed at destroy: the owner table of one pass, key-major, 4 bytes per row and key of the
 * pass and at most 256 MiB (1,024 keys per pass at 65,536 rows); 22 bytes per request of one launch (at most 4 Mi
 * requests); 4 * (7 + max_hops) bytes per key for the census's bins; the point table, the keys and the pair buffers are
 * the ABI 9 buffers, shared. A handle that never calls these launches what it launched and keeps the swimsim_memory
 * figures it had; swimsim_route and swimsim_route_census keep their kernels and results. */
enum { SWIMSIM_FWD_LOCAL = 0, SWIMSIM_FWD_DELIVERED = 1, SWIMSIM_FWD_UNREACHABLE = 2, SWIMSIM_FWD_HOP_LIMIT = 3,
       SWIMSIM_FWD_NO_OWNER = 4, SWIMSIM_FWD_ENTRY_DOWN = 5 };
enum { SWIMSIM_FWD_CHAIN = 0, SWIMSIM_FWD_ONE_HOP = 1 };
int swimsim_forward(swimsim_t *h, const uint8_t *keys, const uint64_t *off, size_t nkeys, uint32_t replica_points,
                    const uint32_t *entry, const uint32_t *key_index, size_t nreq, uint32_t max_hops, int32_t policy,
                    int32_t mode, uint8_t *outcome, uint8_t *hops, int32_t *handler, int32_t *holder, int32_t *next,
                    double *ms);
int swimsim_forward_census(swimsim_t *h, const uint8_t *keys, const uint64_t *off, size_t nkeys, uint32_t replica_points,
                           uint32_t max_hops, int32_t policy, int32_t mode, uint32_t *counted, uint32_t *outcomes,
                           uint32_t *hops_hist, uint64_t *hist_off, int32_t *hist_handler, uint32_t *hist_count,
                           size_t cap, size_t *nhist, double *ms);
int swimsim_forward_times(swimsim_t *h, double *table_ms, double *chase_ms, double *hist_ms);

/* ---- measurement ---- */
/* average device time (ms) of each kernel family since the last reset, for roofline reporting */
int swimsim_kernel_times(swimsim_t *h, const char **names, double *avg_ms, uint64_t *launches,
                         double *alg_bytes, size_t cap, size_t *n);
/* enable: 0 off, 1 every kernel family, 2 only the families the bench line's roofline reports (checksum chains, merges,
 * issue; each timed family costs an event pair per launch in the timed stream) */
int swimsim_enable_timing(swimsim_t *h, int32_t enable);
/* the unit counts behind those byte figures since swimsim_enable_timing (rows hashed by each checksum kernel,
 * changes processed / applied by each merge kernel, records issued, ...): names[i], values[i]; "hot_slots" is
 * the number of hot-column slots in use now (not a count since the reset). "resp_echoed" (ABI 14,
 * swimsim_tuning.resp_echo): direct-ping response records that were kept ("recv_issued" counts them, as do the protocol
 * counter msg_changes and the bump) but not written, being echoes; "resp_merged" no longer counts them, so that
 * resp_merged with resp_echo 0 = resp_merged + resp_echoed with resp_echo 1, and the "alg bytes" of the recv_merge and
 * resp_merge families count fewer processed records than before ABI 14. Three for lazy phase C (ABI 11,
 * swimsim_tuning.cs_defer): "cs_skipped_rounds" = rounds whose phase C hashed nothing, "cs_carried_rows" = the dirty rows
 * they left, summed over those rounds, "cs_forced" = rounds that would have skipped but deferred too many full-sync
 * decisions and hashed. The last one, "bump_by_slot" (ABI 17, swimsim_tuning.slot_bump): the bumps (one per sender message;
 * one per failed helper in phase Q3) taken from the sender's bitmap of sent slots instead of its records; "resp_bumped"
 * counts the records of every bumped direct-ping message either way */
int swimsim_kernel_units(swimsim_t *h, const char **names, double *values, size_t cap, size_t *n);
/* profiler window marker: one tiny kernel (k_profile_mark) on the engine's stream, after the side stream drained */
int swimsim_profile_mark(swimsim_t *h, uint32_t id);
/* time the checksum kernel alone on the first nrows rows — average ms per launch. mode 0: the production choice for
 * nrows rows, 1: the wide kernel (k_checksum3), 2: the narrow kernel (k_checksum_q16), 4: k_checksum3 with four row
 * groups per workgroup, 5: the reference-row path forced (reference row, k_csd_scan, k_csr_rec, k_csr3 and the
 * fallback launches for the rows it leaves), 6: the same on the side stream with its own buffer set (csr2; at most
 * 12,288 rows; SWIMSIM_EINVAL when the set was not allocated). Every other mode is SWIMSIM_EINVAL (up to ABI 11 a
 * diagnostics build, since removed, took more) */
int swimsim_bench_checksum(swimsim_t *h, uint32_t nrows, int32_t mode, int32_t reps, double *ms);
/* the reference-row checksum path so far (swimsim_checksum_ref.hip + swimsim_checksum_csr.hip; swimsim_tuning.cs_ref =
 * 0 off, 1 wide launches, 2 every launch of >= 1024 rows): its launches, the rows it left to the production kernels
 * and, per reason (8 entries: short string, exception-entry capacity, workgroup window plan, record capacity,
 * exception slots of a wave, 5..7 reserved = 0), how many of those rows had it. The counts are kept on the device and
 * read here (no host synchronisation inside a round). */
int swimsim_checksum_path_stats(swimsim_t *h, uint64_t *delta_launches, uint64_t *fallback_rows, uint64_t *reasons);

/* ---- shards: one cluster's observer rows split over G shards ----
 * The reference runs one swim.Node per process; here a shard owns observer rows
 * [N*r/G, N*(r+1)/G) of one simulated cluster and exchanges every cross-shard message (ping
 * requests and responses, ping-req relays, reverse-full-sync and heal memberships) with the other
 * shards at fixed points of the round. With G > 1 swimsim_step() is collective: every shard calls
 * it with the same events. Results stay bit-identical to G = 1. The coverage of the checksum tables is
 * agreed at each step call: a raw write (set_member, set_row, make_change, add_join_list) grows the
 * tables of the shard that owns the row, and the others grow to the largest before a round runs. */
/* G shards in this process (one thread each in swimsim_group_step), all on cfg->device or on
 * devices[i]; copies between shards are device-to-device (peer copies across GPUs) */
int swimsim_group_create(const swimsim_config *cfg, uint32_t nshards, const int32_t *devices, swimsim_t **out);
int swimsim_group_step(swimsim_t *const *handles, uint32_t nshards, uint32_t nrounds, const swimsim_event *events,
                       size_t nevents);
/* one process per GPU: rank 0 makes an id, the launcher broadcasts it, every rank attaches its
 * handle (created with observer_begin/end = its canonical shard); exchanges use RCCL send/recv */
int swimsim_comm_unique_id(uint8_t *out, size_t cap);   /* returns the id length (128) */
int swimsim_comm_attach(swimsim_t *h, uint32_t nranks, uint32_t rank, const uint8_t *id, size_t len);
int swimsim_shard_info(swimsim_t *h, uint32_t *nshards, uint32_t *rank, uint32_t *lo, uint32_t *hi,
                       uint64_t *exchanged_bytes, uint64_t *exchanges);
/* Host synchronisations the cross-shard exchanges of this handle took so far (measurement): one per exchange on the
 * RCCL transport (segment sizes travel on the device behind the pack-size kernel), three on the local and host
 * transports. */
int swimsim_exchange_syncs(swimsim_t *h, uint64_t *syncs);
/* one process per shard with a caller-supplied host transport (any process group: a test harness
 * over gloo, an MPI job, ...). The library stages the packed parcels through host memory and calls:
 *   alltoall_u64: k values to every shard; recv[s*k + i] = shard s's send[rank*k + i]
 *   alltoallv:    segment p of sbuf ([soff[p], soff[p] + sbytes[p])) goes to shard p; the segment
 *                 from shard s lands at rbuf + roff[s] (rbytes[s] bytes, known from a prior alltoall_u64)
 *   bcast:        bytes of shard root to every shard
 * Each returns 0 on success. Same collective call order as the RCCL transport. */
typedef struct swimsim_host_transport {
    void *ctx;
    int (*alltoall_u64)(void *ctx, const uint64_t *send, uint64_t *recv, int32_t k);
    int (*alltoallv)(void *ctx, const uint8_t *sbuf, const uint64_t *soff, const uint64_t *sbytes, uint8_t *rbuf,
                     const uint64_t *roff, const uint64_t *rbytes);
    int (*bcast)(void *ctx, void *buf, size_t bytes, uint32_t root);
} swimsim_host_transport;
int swimsim_comm_attach_host(swimsim_t *h, uint32_t nranks, uint32_t rank, const swimsim_host_transport *t);
/* diagnostics (transport conformance): one collective exchange of caller bytes through the handle's shard
 * transport, exactly as the round's parcel exchange moves them (size exchange, then the segments). send holds
 * the segments for shards 0..G-1 back to back (sbytes[G]); recv receives the segments from shards 0..G-1 back
 * to back (rbytes[G] = their sizes). Every shard calls it. */
int swimsim_debug_exchange(swimsim_t *h, const uint8_t *send, const uint64_t *sbytes, uint8_t *recv, size_t rcap,
                           uint64_t *rbytes);

#ifdef __cplusplus
}
#endif
#endif
