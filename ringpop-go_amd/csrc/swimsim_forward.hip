// swimsim_forward.hip — requests forwarded through every node's own ring view (swimsim_forward, swimsim_forward_census;
// DESIGN.md §17).
//
// A request for key k that enters at node e is handled where owner(h, k) == h and is forwarded to owner(h, k) otherwise
// (Ringpop.HandleOrForward, ringpop.go:687-712), through the ring view of every node it reaches. Two kernels:
//   k_fwd_table   the frame of k_route (one workgroup per row: the presence bitmap, the ascending list, route_owner per
//                 key) with a key-major store: own[(k - k0) * N + row] for the keys [k0, k1) of one pass and every LIVE
//                 row. A chain never holds at a dead node (the entry is checked, a forward needs reach), so a dead
//                 row's cells are never read and its workgroup returns at once.
//   k_fwd_chase   one lane per request. A step is one dependent 4-byte gather of own[k][cur] and one of live and part;
//                 the loop runs at most max_hops + 1 turns. The lanes of a wave share a key wherever the requests
//                 allow it (the census: always), so a wave's gathers stay in one column of 4 * N bytes.
//     listed      writes outcome, hops, handler, holder and next of request i at slot i.
//     census      one workgroup per (key, 256 rows). The outcome and hop bins of the key are counted by ballot and
//                 popcount per wave into LDS and added to the global bins with one integer atomic per non-empty bin and
//                 workgroup. A lane whose handler differs from base[k], the handler under the first counted entry,
//                 stages key << 32 | handler + 1 through the route census's staging frame (route_stage_put,
//                 route_stage_finish); the host sorts and run-length encodes the pairs as for swimsim_route_census.
// The kernels only read mw, live and part, on the main stream.
#pragma once
#include "swimsim_route.hip"

namespace swimdev {

constexpr uint32_t FWD_THREADS = ROUTE_THREADS;
constexpr uint32_t FWD_HOPS_MAX = 64;              // max_hops at most
constexpr uint32_t FWD_NOUT = 6;                   // outcome codes
enum : uint32_t { FWD_LOCAL = 0, FWD_DELIVERED = 1, FWD_UNREACHABLE = 2, FWD_HOP_LIMIT = 3, FWD_NO_OWNER = 4, FWD_ENTRY_DOWN = 5 };

// grid N (the handle owns every row), dynamic LDS route_bitmap_bytes(NP). a.owners is the table, a.k0 / a.k1 the pass.
__global__ void __launch_bounds__(ROUTE_THREADS) k_fwd_table(DS d, RouteArgs a) {
    extern __shared__ unsigned long long route_bm[];
    __shared__ uint32_t list[ROUTE_LIST_CAP];
    __shared__ uint32_t tpre[ROUTE_THREADS];
    __shared__ uint32_t wcnt[ROUTE_THREADS / 64];
    const uint32_t row = blockIdx.x;
    if (row >= d.NL || !d.live[d.lo + row]) return;                    // (the whole workgroup, before any barrier)
    const uint32_t cnt = route_stage_bitmap(d, row, route_bm, wcnt);
    const bool direct = cnt != 0 && route_goes_direct(cnt, a, d.N);
    if (direct) route_stage_list(d, route_bm, list, tpre);             // (the whole workgroup)
    for (uint32_t kb = a.k0; kb < a.k1; kb += ROUTE_THREADS) {
        const uint32_t k = kb + threadIdx.x;
        if (k >= a.k1) break;                                          // (no barrier follows)
        a.owners[(size_t)(k - a.k0) * d.N + row] = cnt ? route_owner(a, route_bm, list, cnt, direct, k) : -1;
    }
}

struct FwdArgs {
    const int32_t *own;              // [k1 - k0][N] the owner table of this pass, key-major
    uint32_t k0, k1;                 // the keys of this pass
    uint32_t max_hops, one_hop;
    // listed: request i of this launch is (ent[i], key[i]); key = nullptr: with j = at + i, (ent[j % nent], k0 + j / nent)
    const uint32_t *ent, *key;
    uint32_t nent, nreq;
    unsigned long long at;
    uint8_t *outcome, *hops;         // (each output may be nullptr)
    int32_t *handler, *holder, *next;
    // census
    const int32_t *base;             // [K] the handler under the first counted entry
    uint32_t *outcomes, *hops_hist;  // [K][6], [K][max_hops + 1]
    RouteArgs r;                     // the staging frame reads exc, cursor and exc_cap
};

struct FwdEnd {
    uint32_t outcome, hops;
    int32_t handler, holder, next;
};

// The chain of one request through column col = own[k][*], from entry e < N. Every node the chain holds at is live: the
// entry is checked here and a forward needs reach, so every cell read was written by k_fwd_table and is -1 or < N.
__device__ __forceinline__ FwdEnd fwd_chase(const DS &d, const int32_t *col, uint32_t e, uint32_t max_hops, bool one_hop) {
    FwdEnd r{FWD_ENTRY_DOWN, 0u, -1, (int32_t)e, -1};
    if (!d.live[e]) return r;
    uint32_t h = e, hops = 0;
    int32_t ph = d.part[e];
    for (;;) {                                                         // (every turn ends the chain or adds a hop)
        const uint32_t to = (uint32_t)col[h];
        if (to >= d.N) { r.outcome = FWD_NO_OWNER; break; }            // (-1: the view is empty)
        if (to == h) { r.outcome = hops ? FWD_DELIVERED : FWD_LOCAL; r.handler = (int32_t)h; break; }
        if (hops == max_hops) { r.outcome = FWD_HOP_LIMIT; r.next = (int32_t)to; break; }
        const int32_t pt = d.part[to];
        if (!d.live[to] || pt != ph) { r.outcome = FWD_UNREACHABLE; r.next = (int32_t)to; break; }
        h = to; ph = pt; hops++;
        if (one_hop) { r.outcome = FWD_DELIVERED; r.handler = (int32_t)h; break; }
    }
    r.holder = (int32_t)h;
    r.hops = hops;
    return r;
}

// listed: grid ceil(nreq / 256). census: grid (k1 - k0) * ceil(N / 256), workgroup b = key k0 + b / nblk, rows
// (b % nblk) * 256 ...
template <bool CENSUS>
__global__ void __launch_bounds__(FWD_THREADS) k_fwd_chase(DS d, FwdArgs a) {
    const uint32_t tid = threadIdx.x;
    if (!CENSUS) {
        const uint32_t i = blockIdx.x * FWD_THREADS + tid;
        if (i >= a.nreq) return;
        uint32_t e, k;
        if (a.key) {
            e = a.ent[i]; k = a.key[i];
        } else {
            const unsigned long long j = a.at + i;
            e = a.ent[j % a.nent]; k = a.k0 + (uint32_t)(j / a.nent);
        }
        const FwdEnd r = fwd_chase(d, a.own + (size_t)(k - a.k0) * d.N, e, a.max_hops, a.one_hop);
        if (a.outcome) a.outcome[i] = (uint8_t)r.outcome;
        if (a.hops) a.hops[i] = (uint8_t)r.hops;
        if (a.handler) a.handler[i] = r.handler;
        if (a.holder) a.holder[i] = r.holder;
        if (a.next) a.next[i] = r.next;
    } else {
        __shared__ uint32_t bins[FWD_NOUT + FWD_HOPS_MAX + 1];
        __shared__ unsigned long long xbuf[FWD_THREADS / 64][ROUTE_STAGE];
        __shared__ uint32_t xcnt[FWD_THREADS / 64];
        __shared__ unsigned long long xat;
        const uint32_t lane = tid & 63u, wave = tid >> 6;
        const uint32_t nblk = (d.N + FWD_THREADS - 1) / FWD_THREADS;
        const uint32_t kk = blockIdx.x / nblk, row = (blockIdx.x - kk * nblk) * FWD_THREADS + tid;
        const uint32_t k = a.k0 + kk, nbin = FWD_NOUT + a.max_hops + 1;
        if (tid < nbin) bins[tid] = 0;
        __syncthreads();
        const bool valid = row < d.N && d.live[row];                   // the entries: every live row
        FwdEnd r{FWD_ENTRY_DOWN, 0u, -1, -1, -1};
        if (valid) r = fwd_chase(d, a.own + (size_t)kk * d.N, row, a.max_hops, a.one_hop);
        // the wave's lanes per outcome and per hop count: one LDS add per value that occurs
        for (uint32_t pass = 0; pass < 2; pass++) {
            const uint32_t v = pass ? FWD_NOUT + r.hops : r.outcome;
            unsigned long long left = __ballot(valid);
            while (left) {                                             // (wave-uniform)
                const uint32_t v0 = (uint32_t)__shfl((int)v, (int)__builtin_ctzll(left));
                const unsigned long long same = __ballot(valid && v == v0);
                if (lane == 0) atomicAdd(&bins[v0], (uint32_t)__popcll(same));
                left &= ~same;
            }
        }
        __syncthreads();
        if (tid < nbin && bins[tid]) {
            if (tid < FWD_NOUT) atomicAdd(&a.outcomes[(size_t)k * FWD_NOUT + tid], bins[tid]);
            else atomicAdd(&a.hops_hist[(size_t)k * (a.max_hops + 1) + (tid - FWD_NOUT)], bins[tid]);
        }
        uint32_t nx = 0;                                               // (one put per wave: the stage never fills)
        route_stage_put(a.r, xbuf[wave], nx, valid && r.handler != a.base[k],
                        [&] { return ((unsigned long long)k << 32) | (uint32_t)(r.handler + 1); }, lane, (1ull << lane) - 1ull);
        route_stage_finish(a.r, xbuf, xcnt, &xat, nx);
    }
}

}  // namespace swimdev
