// swimsim_route.hip — key routing through every observer's own ring view.
//
// The view ring of observer o with R replica points is the ring one AddRemoveServers builds on an empty
// hashring.HashRing from the members row o holds alive or suspect, in ascending member index: its points are
// Fingerprint32(address(m) ‖ decimal(i)), i < R; at an equal hash the lowest present member owns the point; the owner
// of key k is the member of the first point >= Fingerprint32(k) in (hash, member) order, wrapping to the first point;
// an empty ring answers -1. (A real node's ring depends on its history at a shared hash; the view ring is the fresh
// build: include/swimsim.h.)
//
// No ring is built per row. The points of ALL members are hashed and sorted once per R:
//   k_route_points  one lane per (member, replica): hm[m][i] = the hash, pts[m * R + i] = hash << 32 | member;
//                   the host radix-sorts pts, so equal hashes stay, member ascending.
//   k_route_keys    one lane per key: its hash and p0 = the lower bound of the hash in pts (once, not per row).
//   k_route         one workgroup per routed row. It streams the row's words (one dwordx4 per lane) and ballots
//                   status <= suspect into a presence bitmap in LDS (NP / 8 bytes); then one thread per key:
//                     walk    from p0 along pts until a point's member is present (bit test in LDS, never HBM),
//                             wrapping once; expected N / cnt points for a row of cnt servers;
//                     direct  (sparse rows) the present members are listed in LDS in ascending index and the key
//                             takes the minimum of ((hm[m][i] - h) mod 2^32, m) over them and their replicas: the
//                             wrap-around successor with the lowest-member tie-break, cnt * R compares.
//                   Automatic mode takes the direct path while cnt * cnt * R <= N (the walk's N / cnt expected points
//                   cost more than cnt * R compares) and cnt fits the list. Every loop is bounded by N * R.
//                   Census mode: instead of storing owners, a lane whose owner differs from base[k] (the owner under
//                   the first counted row) stages key << 32 | owner + 1 in its wave's LDS buffer; the workgroup
//                   appends what its waves hold with one cursor bump at the end (a wave whose buffer fills flushes
//                   alone, one bump per wave). The host sorts and run-length encodes the pairs, so the result does
//                   not depend on the order of arrival.
//   k_route_n       the same frame, with LookupN per key: the n distinct owners in walk order (below).
// The frame both kernels stand in: route_pick_row (the workgroup's row, or nothing to do), stages 1 and 2
// (route_stage_bitmap, route_stage_list; route_goes_direct chooses the path), and in census mode route_stage_put (a
// wave stages its exception pairs and flushes alone when full) and route_stage_finish (one cursor bump per workgroup).
// Only the search of one key differs: route_owner is k_route's, and k_fwd_table (swimsim_forward.hip) runs
// it in the same frame to fill its key-major owner table.
// The kernels only read mw and live, on the main stream (as the census).
#pragma once
#include "swimsim_device.h"
#include "swimsim_hash.h"

namespace swimdev {

constexpr uint32_t ROUTE_THREADS = 256;            // k_route: 4 waves
constexpr uint32_t ROUTE_GROUP = 256;              // members per wave step (64 lanes x dwordx4) = 4 bitmap words
constexpr uint32_t ROUTE_UNROLL = 4;               // wave steps in flight
constexpr uint32_t ROUTE_LIST_CAP = 512;           // present members the direct path lists in LDS
constexpr uint32_t ROUTE_STAGE = 128;              // census: exception pairs a wave stages in LDS (a key step adds up to 64)
constexpr uint32_t ROUTE_R_MAX = 1000;             // replica strings of 14..23 bytes: one FarmHash length path
constexpr uint32_t ROUTE_N_MAX = 524288;           // the presence bitmap is at most 64 KB of LDS

// LDS bytes of the presence bitmap: 4 words of 64 bits per group of 256 members
__host__ __device__ inline uint32_t route_groups(uint32_t NP) { return (NP + ROUTE_GROUP - 1) / ROUTE_GROUP; }
__host__ __device__ inline uint32_t route_bitmap_bytes(uint32_t NP) { return route_groups(NP) * 32u; }

// Lane l of a wave step loads members c0 .. c0 + 3, c0 = g * 256 + 4 * l, and ballot j holds member c0 + j in bit l:
// member m sits in word (m >> 8) * 4 + (m & 3), bit (m & 255) >> 2.
__device__ __forceinline__ bool route_present(const unsigned long long *bm, uint32_t m) {
    return (bm[(m >> 8) * 4u + (m & 3u)] >> ((m & 255u) >> 2)) & 1ull;
}

// grid ceil(N * R / 256), 256 threads
__global__ void __launch_bounds__(256) k_route_points(const uint32_t *addrw, uint32_t W, uint32_t N, uint32_t R, uint32_t *hm,
                                                      unsigned long long *pts) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= (uint64_t)N * R) return;
    const uint32_t m = (uint32_t)(j / R), i = (uint32_t)(j - (uint64_t)m * R);
    uint8_t name[24], buf[36];                                     // W <= 20 bytes and at most 10 digits
#pragma unroll
    for (uint32_t w = 0; w < 6; w++) {
        const uint32_t x = addrw[(size_t)m * 6 + w];
        name[4 * w] = (uint8_t)x; name[4 * w + 1] = (uint8_t)(x >> 8);
        name[4 * w + 2] = (uint8_t)(x >> 16); name[4 * w + 3] = (uint8_t)(x >> 24);
    }
    const uint32_t len = replica_string(name, W, i, buf);
    buf[len] = buf[len + 1] = buf[len + 2] = buf[len + 3] = 0;
    const uint32_t hash = fp32_dev(buf, len);
    hm[j] = hash;
    pts[j] = ((unsigned long long)hash << 32) | m;
}

// one lane per key (bytes padded with 8 zero bytes: the hash's 4-byte tail reads stay inside)
__global__ void __launch_bounds__(256) k_route_keys(const uint8_t *bytes, const uint64_t *off, uint32_t n,
                                                    const unsigned long long *pts, uint32_t P, uint32_t *kh, uint32_t *p0) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t a = off[k];
    const uint32_t h = fp32_dev(bytes + a, (uint32_t)(off[k + 1] - a));
    kh[k] = h;
    p0[k] = lower_bound_u64(pts, P, (unsigned long long)h << 32);
}

struct RouteArgs {
    const unsigned long long *pts;   // [P] sorted points, hash << 32 | member
    const uint32_t *hm;              // [N][R] replica hashes, member-major
    uint32_t P, R;
    const uint32_t *kh, *p0;         // [K] key hash, lower bound in pts
    uint32_t k0, k1;                 // the keys of this pass
    uint32_t K;                      // row stride of owners
    uint32_t mode;                   // 0 automatic, 1 walk, 2 direct wherever the row fits the list
    const uint32_t *rows;            // route: local row of workgroup b
    int32_t *owners;                 // route: owners[b * K + k]
    const int32_t *base;             // census: [K] owner under the first counted row
    uint32_t skip_row, all;          // census: the first counted row (it is the base), who = all
    unsigned long long *exc;         // census: exception pairs key << 32 | owner + 1
    unsigned long long *cursor;      // census: pairs appended (may pass exc_cap: the pass is re-run over fewer keys)
    unsigned long long exc_cap;
};

// the lanes of a wave read LDS words that other lanes of the same wave wrote
__device__ __forceinline__ void route_fence_lanes() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// lane 0 advances the cursor by n; every lane gets the old value
__device__ __forceinline__ unsigned long long route_bump(unsigned long long *cursor, uint32_t n, uint32_t lane) {
    unsigned long long at = 0;
    if (lane == 0) at = atomicAdd(cursor, (unsigned long long)n);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)at);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(at >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
// a wave copies its n staged pairs to exc[at ...], as far as the buffer goes
__device__ __forceinline__ void route_flush(const RouteArgs &a, const unsigned long long *stage, uint32_t n, unsigned long long at,
                                            uint32_t lane) {
    for (uint32_t i = lane; i < n; i += 64)
        if (at + i < a.exc_cap) a.exc[at + i] = stage[i];
}

// The row of this workgroup; false when it has nothing to do: in census mode the base row and the rows that do not count.
// The caller returns at once: a whole-workgroup return before any barrier.
template <bool CENSUS>
__device__ __forceinline__ bool route_pick_row(const DS &d, const RouteArgs &a, uint32_t &row) {
    if (CENSUS) {
        row = blockIdx.x;
        if (row == a.skip_row || !(a.all || d.live[d.lo + row])) return false;
    } else {
        row = a.rows[blockIdx.x];
    }
    return row < d.NL;
}

// a row of cnt servers takes the direct path: it fits the list, and mode 2 asks for it or mode 0 finds it cheaper
__device__ __forceinline__ bool route_goes_direct(uint32_t cnt, const RouteArgs &a, uint32_t N) {
    return cnt <= ROUTE_LIST_CAP && (a.mode == 2u || (a.mode == 0u && (uint64_t)cnt * cnt * a.R <= N));
}

// Census: the lanes with `is` append pair() to the wave's stage, in lane order; nx, the pairs the wave holds, stays
// wave-uniform. Call it from wave-uniform control flow only (it ballots), with nx <= ROUTE_STAGE - 64: a wave that has no
// room for another 64 pairs afterwards flushes alone. pair is a callable: only the lanes with `is` evaluate it, after
// the ballot. below = (1 << lane) - 1, the lanes before this one: the kernel computes it once, outside its key loop.
template <typename Pair>
__device__ __forceinline__ void route_stage_put(const RouteArgs &a, unsigned long long *stage, uint32_t &nx, bool is, Pair pair,
                                                uint32_t lane, unsigned long long below) {
    const unsigned long long mask = __ballot(is);
    if (!mask) return;
    if (is) stage[nx + (uint32_t)__popcll(mask & below)] = pair();
    nx += (uint32_t)__popcll(mask);
    if (nx > ROUTE_STAGE - 64) {
        route_fence_lanes();
        route_flush(a, stage, nx, route_bump(a.cursor, nx, lane), lane);
        route_fence_lanes();
        nx = 0;
    }
}

// Census, the whole workgroup after its last key step: what the waves still hold is appended with one cursor bump.
// xcnt: ROUTE_THREADS / 64 words; xat: one word.
__device__ __forceinline__ void route_stage_finish(const RouteArgs &a, const unsigned long long (*xbuf)[ROUTE_STAGE], uint32_t *xcnt,
                                                   unsigned long long *xat, uint32_t nx) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (lane == 0) xcnt[wave] = nx;
    __syncthreads();
    if (tid == 0) {
        uint32_t tot = 0;
#pragma unroll
        for (uint32_t v = 0; v < ROUTE_THREADS / 64; v++) tot += xcnt[v];
        *xat = tot ? atomicAdd(a.cursor, (unsigned long long)tot) : 0ull;
    }
    __syncthreads();
    unsigned long long at = *xat;
    for (uint32_t v = 0; v < wave; v++) at += xcnt[v];
    route_flush(a, xbuf[wave], nx, at, lane);
}

// Stage 1 of a routed row (the whole workgroup, ROUTE_THREADS threads): stream the row's words and ballot status <= suspect
// into the presence bitmap route_bm (route_bitmap_bytes(NP) of LDS). Returns cnt, the row's servers. wcnt: ROUTE_THREADS / 64 words.
__device__ __forceinline__ uint32_t route_stage_bitmap(const DS &d, uint32_t row, unsigned long long *route_bm, uint32_t *wcnt) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t *rowp = d.mw + (size_t)row * d.NP;
    const uint32_t ngroups = route_groups(d.NP);
    uint32_t cntw = 0;
    for (uint32_t g0 = wave * ROUTE_UNROLL; g0 < ngroups; g0 += (ROUTE_THREADS / 64) * ROUTE_UNROLL) {
        uint4 w[ROUTE_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < ROUTE_UNROLL; u++) {
            const uint32_t c0 = (g0 + u) * ROUTE_GROUP + lane * 4u;    // NP is a multiple of 64: c0 < NP covers c0 + 3
            w[u] = c0 < d.NP ? *reinterpret_cast<const uint4 *>(rowp + c0) : make_uint4(ST_UNKNOWN, ST_UNKNOWN, ST_UNKNOWN, ST_UNKNOWN);
        }
#pragma unroll
        for (uint32_t u = 0; u < ROUTE_UNROLL; u++) {
            const uint32_t g = g0 + u;
            if (g >= ngroups) break;                                   // (wave-uniform)
            const uint32_t c0 = g * ROUTE_GROUP + lane * 4u;
            const unsigned long long b0 = __ballot(c0 < d.N && (w[u].x & 7u) <= ST_SUSPECT);
            const unsigned long long b1 = __ballot(c0 + 1 < d.N && (w[u].y & 7u) <= ST_SUSPECT);
            const unsigned long long b2 = __ballot(c0 + 2 < d.N && (w[u].z & 7u) <= ST_SUSPECT);
            const unsigned long long b3 = __ballot(c0 + 3 < d.N && (w[u].w & 7u) <= ST_SUSPECT);
            if (lane == 0) {
                route_bm[g * 4u] = b0; route_bm[g * 4u + 1] = b1; route_bm[g * 4u + 2] = b2; route_bm[g * 4u + 3] = b3;
            }
            cntw += (uint32_t)(__popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3));
        }
    }
    if (lane == 0) wcnt[wave] = cntw;
    __syncthreads();
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t v = 0; v < ROUTE_THREADS / 64; v++) cnt += wcnt[v];
    return cnt;
}

// Stage 2 (the whole workgroup): the present members as a list in LDS, ascending, as far as ROUTE_LIST_CAP goes.
// tpre: ROUTE_THREADS words.
__device__ __forceinline__ void route_stage_list(const DS &d, const unsigned long long *route_bm, uint32_t *list, uint32_t *tpre) {
    const uint32_t tid = threadIdx.x;
    const uint32_t ngroups = route_groups(d.NP);
    const uint32_t gper = (ngroups + ROUTE_THREADS - 1) / ROUTE_THREADS;
    const uint32_t gs = min(tid * gper, ngroups), ge = min(gs + gper, ngroups);
    uint32_t mine = 0;
    for (uint32_t g = gs; g < ge; g++)
        mine += (uint32_t)(__popcll(route_bm[g * 4u]) + __popcll(route_bm[g * 4u + 1]) + __popcll(route_bm[g * 4u + 2]) +
                           __popcll(route_bm[g * 4u + 3]));
    tpre[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (uint32_t t = 0; t < ROUTE_THREADS; t++) {
            const uint32_t c = tpre[t];
            tpre[t] = run;
            run += c;
        }
    }
    __syncthreads();
    uint32_t at = tpre[tid];
    for (uint32_t g = gs; g < ge; g++) {
        const unsigned long long b0 = route_bm[g * 4u], b1 = route_bm[g * 4u + 1], b2 = route_bm[g * 4u + 2],
                                 b3 = route_bm[g * 4u + 3];
        unsigned long long any = b0 | b1 | b2 | b3;
        while (any) {
            const uint32_t l = (uint32_t)__builtin_ctzll(any);
            any &= any - 1;
            const uint32_t m = g * ROUTE_GROUP + l * 4u;
            if ((b0 >> l) & 1ull) { if (at < ROUTE_LIST_CAP) list[at] = m; at++; }
            if ((b1 >> l) & 1ull) { if (at < ROUTE_LIST_CAP) list[at] = m + 1; at++; }
            if ((b2 >> l) & 1ull) { if (at < ROUTE_LIST_CAP) list[at] = m + 2; at++; }
            if ((b3 >> l) & 1ull) { if (at < ROUTE_LIST_CAP) list[at] = m + 3; at++; }
        }
    }
    __syncthreads();
}

// Stage 3, one thread: the owner of key k in a row of cnt > 0 servers, by the path stages 1 and 2 prepared. Every lane of
// a wave that takes the direct path is at the same list index (the readfirstlane below).
__device__ __forceinline__ int32_t route_owner(const RouteArgs &a, const unsigned long long *route_bm, const uint32_t *list,
                                               uint32_t cnt, bool direct, uint32_t k) {
    const uint32_t h = a.kh[k];
    if (direct) {
        unsigned long long best = ~0ull;
        for (uint32_t j = 0; j < cnt; j++) {
            const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[j]);
            const uint32_t *hp = a.hm + (size_t)m * a.R;
            for (uint32_t i = 0; i < a.R; i++) {
                const unsigned long long v = ((unsigned long long)(hp[i] - h) << 32) | m;
                best = v < best ? v : best;
            }
        }
        return (int32_t)(uint32_t)best;
    }
    const uint32_t *ptm = reinterpret_cast<const uint32_t *>(a.pts);   // (the member is the low word of a point)
    uint32_t p = a.p0[k];
    for (uint32_t step = 0; step < a.P; step++, p++) {                 // cnt > 0: a present member's point is met
        if (p >= a.P) p = 0;
        const uint32_t m = ptm[2 * (size_t)p];
        if (route_present(route_bm, m)) return (int32_t)m;
    }
    return -1;
}

// route: grid = routed rows; census: grid = NL (workgroups of rows that do not count return at once).
// Dynamic LDS: route_bitmap_bytes(NP).
template <bool CENSUS>
__global__ void __launch_bounds__(ROUTE_THREADS) k_route(DS d, RouteArgs a) {
    extern __shared__ unsigned long long route_bm[];
    __shared__ uint32_t list[ROUTE_LIST_CAP];
    __shared__ uint32_t tpre[ROUTE_THREADS];
    __shared__ uint32_t wcnt[ROUTE_THREADS / 64];
    __shared__ unsigned long long xbuf[ROUTE_THREADS / 64][ROUTE_STAGE];   // census: each wave's exception pairs
    __shared__ uint32_t xcnt[ROUTE_THREADS / 64];
    __shared__ unsigned long long xat;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t row;
    if (!route_pick_row<CENSUS>(d, a, row)) return;                    // (the whole workgroup, before any barrier)
    // ---- 1. the presence bitmap of the row ----
    const uint32_t cnt = route_stage_bitmap(d, row, route_bm, wcnt);
    // ---- 2. sparse rows: the present members as a list, ascending ----
    const bool direct = cnt != 0 && route_goes_direct(cnt, a, d.N);
    if (direct) route_stage_list(d, route_bm, list, tpre);             // (the whole workgroup)
    // ---- 3. one thread per key ----
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t nx = 0;                                                   // census: pairs staged by this wave (wave-uniform)
    for (uint32_t kb = a.k0; kb < a.k1; kb += ROUTE_THREADS) {         // (kb + tid < 2^32: k1 <= 2^31)
        const uint32_t k = kb + tid;
        const bool valid = k < a.k1;
        const int32_t own = valid && cnt ? route_owner(a, route_bm, list, cnt, direct, k) : -1;
        if (!CENSUS) {
            if (valid) a.owners[(size_t)blockIdx.x * a.K + k] = own;
        } else {                                                       // (every lane is here: one put per key step)
            route_stage_put(a, xbuf[wave], nx, valid && own != a.base[k],
                            [&] { return ((unsigned long long)k << 32) | (uint32_t)(own + 1); }, lane, below);
        }
    }
    if (CENSUS) route_stage_finish(a, xbuf, xcnt, &xat, nx);
}

// ---- replica sets: LookupN through every observer's view (swimsim_route_n / swimsim_replica_census) ----
//
// prefs(o, k, n): the n distinct owners the view ring of observer o meets from the first REAL point >= Fingerprint32(k),
// wrapping once, each at its first occurrence; a view of cnt <= n servers lists all of them in ascending member index
// (include/swimsim.h). A point is real only for the lowest present member at its hash: pts and hm hold an entry for
// every member, so when present members a < b share a hash, b's entry is no point of this view and must not list b.
//   k_route_n   the frame of k_route (the row pick, the presence bitmap, the ascending list), then one thread per key:
//     cnt <= n  the list itself (n <= ROUTE_NN_MAX <= ROUTE_LIST_CAP: such a row always fits the list);
//     walk      from p0 along pts, the whole 8-byte point. A point whose member is present is taken unless its hash
//               equals the hash of the last present point seen (equal hashes are contiguous in pts, member ascending,
//               and p0 is a lower bound, so a run is never entered in its middle: the first present entry of a run is
//               the real point, every later present entry a duplicate, whether or not the first one's member was new),
//               and unless its member is already collected. Stops at n members, at most P steps, one wrap;
//     direct    the same walk over the listed members' own replica hashes: each step takes the minimum of
//               ((hm[m][i] - h) mod 2^32) << 32 | m above the last one taken, over ALL listed members (collected ones
//               too: a collected member's entry at a shared hash is what marks the higher member's entry a
//               duplicate), cnt * R compares per step. Walk and direct visit the same present points, so the
//               ratio of their costs is ABI 9's: direct while cnt * cnt * R <= N.
//   The collected members of a thread are n words of LDS, coll[i * ROUTE_THREADS + tid] (16 KB at n = 16: with the
//   64 KB bitmap of N = 524,288, the list, the prefix and the stage that is 87 KB of a CU's 160 KB).
//   Census: base[k * n + i] is the set under the first counted row. A lane whose set differs stages
//   key << 32 | (member + 1) << 1 | sign for every member of its set that is not in the base (sign 0) and every base
//   member that is not in its set (sign 1): up to 2n pairs per key and row. The pairs of a key step are staged slot by
//   slot (2n ballots, each adds up to 64 pairs to the wave's buffer, which flushes when another 64 would not fit), so
//   ROUTE_STAGE holds as it is. A pass over ONE key appends at most 2n * NL pairs: the host sizes the buffer to at
//   least that, so that halving the keys of an overflowing pass always ends (swimsim_replica_census).
constexpr uint32_t ROUTE_NN_MAX = 16;              // replicas per key at most (the n of LookupN)
static_assert(ROUTE_NN_MAX <= ROUTE_LIST_CAP && 2 * ROUTE_NN_MAX <= 32, "a row of cnt <= n fits the list; 2n slot bits");
// static LDS of k_route_n (the dynamic bitmap comes on top): coll, list, tpre, xbuf and the small words
constexpr uint32_t ROUTE_N_STATIC_LDS = ROUTE_NN_MAX * ROUTE_THREADS * 4 + ROUTE_LIST_CAP * 4 + ROUTE_THREADS * 4 +
                                        (ROUTE_THREADS / 64) * ROUTE_STAGE * 8 + 64;

struct RouteNArgs {
    RouteArgs r;                     // owners, base and K are not used
    uint32_t n;                      // 1..ROUTE_NN_MAX
    int32_t *prefs;                  // route: prefs[(b * K + k) * n + i], -1 past min(n, cnt)
    uint32_t *servers;               // route: servers[b] = cnt
    const int32_t *nbase;            // census: [K][n] the set under the first counted row, -1 past min(n, cnt)
};

// route: grid = routed rows; census: grid = NL. Dynamic LDS: route_bitmap_bytes(NP).
template <bool CENSUS>
__global__ void __launch_bounds__(ROUTE_THREADS) k_route_n(DS d, RouteNArgs an) {
    extern __shared__ unsigned long long route_bm[];
    __shared__ uint32_t coll[ROUTE_NN_MAX * ROUTE_THREADS];
    __shared__ uint32_t list[ROUTE_LIST_CAP];
    __shared__ uint32_t tpre[ROUTE_THREADS];
    __shared__ uint32_t wcnt[ROUTE_THREADS / 64];
    __shared__ unsigned long long xbuf[ROUTE_THREADS / 64][ROUTE_STAGE];
    __shared__ uint32_t xcnt[ROUTE_THREADS / 64];
    __shared__ unsigned long long xat;
    const RouteArgs &a = an.r;
    const uint32_t n = an.n;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t row;
    if (!route_pick_row<CENSUS>(d, a, row)) return;                    // (the whole workgroup, before any barrier)
    const uint32_t cnt = route_stage_bitmap(d, row, route_bm, wcnt);
    const bool small = cnt <= n;                                       // every server, ascending: the list
    const bool direct = !small && route_goes_direct(cnt, a, d.N);
    if (cnt != 0 && (small || direct)) route_stage_list(d, route_bm, list, tpre);   // (the whole workgroup)
    if (!CENSUS && tid == 0 && an.servers) an.servers[blockIdx.x] = cnt;
    const uint32_t want = min(n, cnt);
    uint32_t *mine = coll + tid;                                       // member i of this thread: mine[i * ROUTE_THREADS]
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t nx = 0;                                                   // census: pairs staged by this wave (wave-uniform)
    for (uint32_t kb = a.k0; kb < a.k1; kb += ROUTE_THREADS) {
        const uint32_t k = kb + tid;
        const bool valid = k < a.k1;
        uint32_t got = 0;
        if (valid && cnt) {
            const uint32_t h = a.kh[k];
            if (small) {
                for (; got < cnt; got++) mine[got * ROUTE_THREADS] = list[got];
            } else if (direct) {
                unsigned long long cur = 0;                            // the last (distance, member) taken
                bool first = true;
                uint32_t lastd = 0;
                for (uint32_t step = 0; step < a.P && got < want; step++) {
                    unsigned long long best = ~0ull;
                    for (uint32_t j = 0; j < cnt; j++) {
                        const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[j]);   // (j is the same in every active lane)
                        const uint32_t *hp = a.hm + (size_t)m * a.R;
                        for (uint32_t i = 0; i < a.R; i++) {
                            const unsigned long long v = ((unsigned long long)(hp[i] - h) << 32) | m;
                            if ((first || v > cur) && v < best) best = v;
                        }
                    }
                    if (best == ~0ull) break;                          // every entry was visited
                    const uint32_t dist = (uint32_t)(best >> 32), m = (uint32_t)best;
                    const bool dup = !first && dist == lastd;          // a higher member's entry at the same hash
                    cur = best; first = false; lastd = dist;
                    if (!dup) {
                        bool seen = false;
                        for (uint32_t q = 0; q < got; q++) seen |= mine[q * ROUTE_THREADS] == m;
                        if (!seen) mine[got++ * ROUTE_THREADS] = m;
                    }
                }
            } else {
                uint32_t p = a.p0[k], lasth = 0;
                bool any = false;                                      // a present point was seen: lasth holds its hash
                for (uint32_t step = 0; step < a.P && got < want; step++, p++) {
                    if (p >= a.P) p = 0;
                    const unsigned long long pt = a.pts[p];
                    const uint32_t m = (uint32_t)pt, ph = (uint32_t)(pt >> 32);
                    if (!route_present(route_bm, m)) continue;
                    const bool dup = any && ph == lasth;
                    any = true; lasth = ph;
                    if (dup) continue;
                    bool seen = false;
                    for (uint32_t q = 0; q < got; q++) seen |= mine[q * ROUTE_THREADS] == m;
                    if (!seen) mine[got++ * ROUTE_THREADS] = m;
                }
            }
        }
        if (!CENSUS) {
            if (valid) {
                int32_t *out = an.prefs + ((size_t)blockIdx.x * a.K + k) * n;
                for (uint32_t i = 0; i < n; i++) out[i] = i < got ? (int32_t)mine[i * ROUTE_THREADS] : -1;
            }
        } else {
            uint32_t plus = 0, minus = 0;                              // bit i: my member i is not in the base; base member i not mine
            const int32_t *bp = an.nbase + (size_t)(valid ? k : a.k0) * n;
            if (valid) {
                bool same = true;
                for (uint32_t i = 0; i < n; i++) same &= bp[i] == (i < got ? (int32_t)mine[i * ROUTE_THREADS] : -1);
                if (!same) {                                           // (equal lists are equal sets: the common case)
                    for (uint32_t i = 0; i < got; i++) {
                        const int32_t m = (int32_t)mine[i * ROUTE_THREADS];
                        bool in = false;
                        for (uint32_t j = 0; j < n; j++) in |= bp[j] == m;
                        if (!in) plus |= 1u << i;
                    }
                    for (uint32_t j = 0; j < n; j++) {
                        const int32_t b = bp[j];
                        if (b < 0) break;                              // (the base's -1 slots are its last)
                        bool in = false;
                        for (uint32_t i = 0; i < got; i++) in |= (int32_t)mine[i * ROUTE_THREADS] == b;
                        if (!in) minus |= 1u << j;
                    }
                }
            }
            if (__ballot((plus | minus) != 0u)) {                      // (wave-uniform)
                for (uint32_t s = 0; s < 2u * n; s++) {                // (one put per slot: each adds up to 64 pairs)
                    const bool sign = s >= n;
                    const uint32_t i = sign ? s - n : s;
                    // (the slot's member: base member i or my member i; one pointer, read only by the lanes that stage)
                    const uint32_t *src = sign ? reinterpret_cast<const uint32_t *>(bp) + i : mine + i * ROUTE_THREADS;
                    route_stage_put(a, xbuf[wave], nx, ((sign ? minus : plus) >> i) & 1u, [&] {
                        const uint32_t m = *src;
                        return ((unsigned long long)k << 32) | ((unsigned long long)(m + 1u) << 1) | (sign ? 1ull : 0ull);
                    }, lane, below);
                }
            }
        }
    }
    if (CENSUS) route_stage_finish(a, xbuf, xcnt, &xat, nx);
}

}  // namespace swimdev
