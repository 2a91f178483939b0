"""Failure-detection metrics from a member trace (Cluster.trace / ShardedCluster.trace) and routing agreement from
a route census (Cluster.route_census / ShardedCluster.route_census) or a replica census (replica_census).

Plain numpy on the trace arrays: no device, no library. The status columns of a census count are alive, suspect,
faulty, leave, tombstone, unknown (swimsim.CENSUS_STATUSES).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

ALIVE, SUSPECT, FAULTY, LEAVE, TOMBSTONE, UNKNOWN = range(6)


@dataclass
class DetectionTimes:
    """per tracked member, the recorded round (None: never in the trace) in which
    first_suspect: some live observer first held it suspect or worse (suspect, faulty, leave, tombstone);
    first_faulty:  some live observer first held it faulty or worse (faulty, leave, tombstone);
    all_faulty:    every live observer first held it faulty or worse, or no longer knew it (unknown: evicted)."""
    first_suspect: list
    first_faulty: list
    all_faulty: list


def _first(rounds, hit) -> list:
    """per column of hit[k, n], the round of the first true entry"""
    out: list = []
    for j in range(hit.shape[1]):
        ks = np.nonzero(hit[:, j])[0]
        out.append(int(rounds[ks[0]]) if len(ks) else None)
    return out


def detection_times(rounds, nlive, counts) -> DetectionTimes:
    """rounds[k], nlive[k], counts[k, n, 6] as trace() returns them (live observer rows). Rounds are looked at in the
    order recorded; a gap in `rounds` (records dropped by a full buffer) is simply not seen: the answer is the first
    RECORDED round. A round with no live observer detects nothing."""
    rounds = np.asarray(rounds).reshape(-1)
    nlive = np.asarray(nlive, dtype=np.int64).reshape(-1)
    counts = np.asarray(counts, dtype=np.int64)
    if counts.ndim != 3 or counts.shape[2] != 6 or counts.shape[0] != len(rounds) or len(nlive) != len(rounds):
        raise ValueError("detection_times: rounds[k], nlive[k] and counts[k, n, 6] expected")
    suspect_up = counts[:, :, SUSPECT:TOMBSTONE + 1].sum(axis=2)
    faulty_up = counts[:, :, FAULTY:TOMBSTONE + 1].sum(axis=2)
    gone = faulty_up + counts[:, :, UNKNOWN]
    some_live = (nlive > 0)[:, None]
    return DetectionTimes(_first(rounds, suspect_up > 0), _first(rounds, faulty_up > 0),
                          _first(rounds, (gone == nlive[:, None]) & some_live))


@dataclass
class RouteAgreement:
    """per key of a route census:
    distinct:  the number of distinct owners the counted rows answer (0: no row counted);
    owner:     the plurality owner, the lowest owner among equals (-1 is an owner: the empty ring; -2: no row counted);
    count:     the number of counted rows that answer the plurality owner."""
    distinct: np.ndarray
    owner: np.ndarray
    count: np.ndarray

    def agreed(self, counted) -> np.ndarray:
        """per key: every counted row answers the same owner"""
        return self.count == counted


def route_agreement(counted, hist_off, hist_owner, hist_count) -> RouteAgreement:
    """counted, hist_off[K + 1], hist_owner, hist_count as route_census() returns them (owners ascending per key)."""
    hist_off = np.asarray(hist_off, dtype=np.int64).reshape(-1)
    hist_owner = np.asarray(hist_owner, dtype=np.int64).reshape(-1)
    hist_count = np.asarray(hist_count, dtype=np.int64).reshape(-1)
    if len(hist_off) < 1 or len(hist_owner) != len(hist_count) or (len(hist_off) and hist_off[-1] != len(hist_owner)):
        raise ValueError("route_agreement: hist_off[K + 1] and hist_owner / hist_count of hist_off[K] entries expected")
    K = len(hist_off) - 1
    distinct = np.diff(hist_off)
    owner = np.full(K, -2, np.int64)
    count = np.zeros(K, np.int64)
    for k in range(K):
        a, b = hist_off[k], hist_off[k + 1]
        if b > a:
            j = a + int(np.argmax(hist_count[a:b]))                  # (argmax takes the first: the lowest owner)
            owner[k], count[k] = hist_owner[j], hist_count[j]
    return RouteAgreement(distinct, owner, count)


@dataclass
class RingAgreement:
    """of a ring census (the ring.checksum gauge over the counted rows):
    distinct:  the number of distinct ring checksums the counted rows answer (0: no row counted);
    checksum:  the majority checksum, the lowest value among equals (None: no row counted);
    share:     the fraction of the counted rows that answer it (0.0: no row counted);
    all_agree: every counted row answers the same checksum (False when no row counted)."""
    distinct: int
    checksum: int | None
    share: float
    all_agree: bool


def ring_agreement(counted, hist_checksum, hist_count) -> RingAgreement:
    """counted, hist_checksum, hist_count as ring_census() returns them (checksums ascending, counts summing to counted)."""
    cs = np.asarray(hist_checksum, dtype=np.int64).reshape(-1)
    cnt = np.asarray(hist_count, dtype=np.int64).reshape(-1)
    if len(cs) != len(cnt) or int(cnt.sum()) != int(counted) or (len(cs) > 1 and (np.diff(cs) <= 0).any()) or (cnt <= 0).any():
        raise ValueError("ring_agreement: ascending distinct checksums with positive counts that sum to counted expected")
    if not len(cs):
        return RingAgreement(0, None, 0.0, False)
    j = int(np.argmax(cnt))                                          # (argmax takes the first: the lowest checksum)
    return RingAgreement(len(cs), int(cs[j]), float(cnt[j]) / float(counted), len(cs) == 1)


@dataclass
class ReplicaAgreement:
    """per key of a replica census with sets of n members:
    distinct:   the number of distinct members over the counted rows' replica sets;
    unanimous:  the number of members every counted row lists (count = counted);
    agreed:     every counted row holds the same replica set (every listed member is unanimous; true for a key
                with no entry: no row counted, or every counted view empty)."""
    distinct: np.ndarray
    unanimous: np.ndarray
    agreed: np.ndarray


def replica_agreement(counted, hist_off, hist_member, hist_count, n) -> ReplicaAgreement:
    """counted, hist_off[K + 1], hist_member, hist_count as replica_census(keys, n) returns them."""
    hist_off = np.asarray(hist_off, dtype=np.int64).reshape(-1)
    hist_member = np.asarray(hist_member, dtype=np.int64).reshape(-1)
    hist_count = np.asarray(hist_count, dtype=np.int64).reshape(-1)
    if len(hist_off) < 1 or len(hist_member) != len(hist_count) or hist_off[-1] != len(hist_member):
        raise ValueError("replica_agreement: hist_off[K + 1] and hist_member / hist_count of hist_off[K] entries expected")
    if not 1 <= int(n) <= 16:
        raise ValueError(f"replica_agreement: n is 1..16, not {n!r}")
    if len(hist_count) and (hist_count.min() < 1 or hist_count.max() > int(counted)):
        raise ValueError("replica_agreement: every count is 1..counted")
    K = len(hist_off) - 1
    distinct = np.diff(hist_off)
    full = np.concatenate([[0], np.cumsum(hist_count == int(counted))])
    unanimous = full[hist_off[1:]] - full[hist_off[:-1]]
    if (unanimous > int(n)).any():
        raise ValueError(f"replica_agreement: a key lists more than n = {n} members in every counted row")
    return ReplicaAgreement(distinct, unanimous, unanimous == distinct)


@dataclass
class ForwardAvailability:
    """per key of a forward census (requests forwarded through every live node's own ring view):
    served:      the share of the counted entries whose request is handled, LOCAL or DELIVERED (0.0: no entry counted);
    mean_hops:   the mean number of forwards of the served requests (nan: none served). The hop bins hold every
                 request, served or not: a HOP_LIMIT request made max_hops forwards and is taken out, an UNREACHABLE or
                 NO_OWNER request may have ended at any hop, so for a key that has such requests the figure is an upper
                 bound (they are taken as ending at hop 0) and hops_exact is False;
    hops_exact:  mean_hops is exact: the key has no UNREACHABLE and no NO_OWNER request;
    handlers:    the number of distinct nodes that handle the key;
    split:       more than one node handles the key;
    and the totals over all keys: requests = counted * K, served_total, outcome_totals[6] in the order of the outcome
    codes (local, delivered, unreachable, hop_limit, no_owner, entry_down), hops_total[max_hops + 1], split_keys."""
    served: np.ndarray
    mean_hops: np.ndarray
    hops_exact: np.ndarray
    handlers: np.ndarray
    split: np.ndarray
    requests: int
    served_total: int
    outcome_totals: np.ndarray
    hops_total: np.ndarray
    split_keys: int


def forward_availability(counted, outcomes, hops_hist, hist_off, hist_handler, hist_count) -> ForwardAvailability:
    """counted, outcomes[K, 6], hops_hist[K, max_hops + 1], hist_off[K + 1], hist_handler, hist_count as forward_census()
    returns them (handlers ascending per key, -1 = not served first)."""
    counted = int(counted)
    outcomes = np.asarray(outcomes, dtype=np.int64)
    hops_hist = np.asarray(hops_hist, dtype=np.int64)
    hist_off = np.asarray(hist_off, dtype=np.int64).reshape(-1)
    hist_handler = np.asarray(hist_handler, dtype=np.int64).reshape(-1)
    hist_count = np.asarray(hist_count, dtype=np.int64).reshape(-1)
    K = len(hist_off) - 1
    if K < 0 or outcomes.shape != (K, 6) or hops_hist.ndim != 2 or len(hops_hist) != K or hops_hist.shape[1] < 2 or \
            len(hist_handler) != len(hist_count) or hist_off[-1] != len(hist_handler):
        raise ValueError("forward_availability: outcomes[K, 6], hops_hist[K, max_hops + 1], hist_off[K + 1] and hist_handler / "
                         "hist_count of hist_off[K] entries expected")
    key = np.repeat(np.arange(K), np.diff(hist_off))
    per_key = lambda sel: np.bincount(key[sel], weights=hist_count[sel], minlength=K).astype(np.int64)
    good = outcomes[:, 0] + outcomes[:, 1]
    if (outcomes.sum(axis=1) != counted).any() or (hops_hist.sum(axis=1) != counted).any() or \
            (per_key(hist_handler >= 0) != good).any() or (per_key(hist_handler < 0) != counted - good).any():
        raise ValueError("forward_availability: per key, the outcome bins, the hop bins and the handler counts sum to counted, "
                         "and the handlers >= 0 take the local and delivered requests")
    max_hops = hops_hist.shape[1] - 1
    hops = (hops_hist * np.arange(max_hops + 1)).sum(axis=1) - max_hops * outcomes[:, 3]
    handlers = np.bincount(key[hist_handler >= 0], minlength=K)
    return ForwardAvailability(served=good / counted if counted else np.zeros(K),
                               mean_hops=np.where(good > 0, hops / np.maximum(good, 1), np.nan),
                               hops_exact=outcomes[:, 2] + outcomes[:, 4] == 0, handlers=handlers, split=handlers > 1,
                               requests=counted * K, served_total=int(good.sum()), outcome_totals=outcomes.sum(axis=0),
                               hops_total=hops_hist.sum(axis=0), split_keys=int((handlers > 1).sum()))
