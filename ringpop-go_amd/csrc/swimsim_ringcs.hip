// swimsim_ringcs.hip — the ring checksum of every observer's own ring view.
//
// ringcs(o) = Fingerprint32(S), S = the addresses of the members row o holds alive or suspect, in ascending member
// index, joined by ';' (Ringpop.Checksum, ringpop.go:571-577; hashring.go:100-107). Addresses are fixed-width
// (W = 13..20) and ascending, so S is cnt records of W + 1 bytes less the last ';': len = cnt * (W + 1) - 1, and record r
// starts at byte r * (W + 1). It is not the membership checksum: no incarnation and no status enters it.
//
//   k_ringcs_scan    one workgroup per requested row: route_stage_bitmap gives the presence bitmap in LDS and cnt; the
//                    workgroup reduces key = the sum of ringcs_mix(m) over the present members (order-free, 64 bits)
//                    and writes (key, cnt). The host groups rows of equal (key, cnt) under their lowest row.
//   k_ringcs_verify  one workgroup per grouped row that is not its group's representative: it streams both rows' words
//                    again and compares presence member by member (nothing of the scan is stored). A row that differs
//                    is hashed on its own, so a key collision costs a chain and never a wrong checksum.
//   k_ringcs_hash    one workgroup per representative. S is never written to HBM. The row's bitmap is staged as in the
//                    scan, then expanded RINGCS_CHUNK member indices at a time: thread t owns four member indices of
//                    the chunk, ranks its present ones by popcounts of the chunk's bitmap words and writes their
//                    records (address bytes from addrw, 24 B per member, and the ';') at their string positions into
//                    a byte ring in LDS. Blocks start at multiples of 20 bytes, so every word of a block is an aligned
//                    word of that ring. A block is ready when its 20 bytes and the 12 bytes of look-ahead are in the
//                    ring (the last block: when the string is complete, its look-ahead zero). Waves 1..3 premix
//                    the ready blocks in batches of RINGCS_NB into the carried-sum form of swimsim_checksum4.hip
//                    ({M, K} per chain lane: the three M() terms of FH::block and the folded constants), double
//                    buffered against the chain, which lanes 0..3 of wave 0 run with fh_quad_step (g, f, h, 0).
//                    FH::init takes the last 20 bytes of S, which the highest present members give before the chain
//                    starts. cnt <= 1 (the empty string, one address of 13..20 bytes) takes fp32_dev directly.
//   k_ringcs_scatter every requested row takes its representative's checksum.
// Every loop is bounded by cnt, N or the bitmap's words; a whole workgroup returns before any barrier. Static LDS of
// the hash kernel: the byte ring (21,760 B), two premix buffers (8 KB) and a few words, on top of the bitmap.
// The kernels only read mw and addrw, on the main stream (as the route kernels).
#pragma once
#include "swimsim_route.hip"

namespace swimdev {

constexpr uint32_t RINGCS_THREADS = ROUTE_THREADS;           // route_stage_bitmap's workgroup
constexpr uint32_t RINGCS_CHUNK = 1024;                      // member indices per expansion step: 4 bitmap groups
constexpr uint32_t RINGCS_NB = 128;                          // blocks per premix batch
constexpr uint32_t RINGCS_HOLD = 32;                         // bytes a ready block needs in the ring: its 20 and 12 of look-ahead
constexpr uint32_t RINGCS_RB = 21760;                        // byte ring: a chunk of 21-byte records, the hold, in whole blocks
constexpr uint32_t RINGCS_RBW = RINGCS_RB / 4;
constexpr uint32_t RINGCS_STATIC_LDS = RINGCS_RB + 2 * RINGCS_NB * 4 * 8 + 64;
static_assert(RINGCS_CHUNK == 4 * ROUTE_GROUP && RINGCS_THREADS == 256, "a thread owns 4 member indices of a chunk");
static_assert(RINGCS_RB % 20 == 0 && RINGCS_RB >= RINGCS_CHUNK * 21 + RINGCS_HOLD + 4, "the ring holds a chunk and the hold");
static_assert(RINGCS_STATIC_LDS <= 32768, "LDS beside the bitmap");

// per-member term of a view's grouping key: a function of the member index alone
__host__ __device__ inline unsigned long long ringcs_mix(uint32_t m) {
    return fmix64(((unsigned long long)m + 1ull) * 0x9E3779B97F4A7C15ULL);
}

__device__ __forceinline__ uint32_t ringcs_addr_byte(const DS &d, uint32_t m, uint32_t k) {
    return reinterpret_cast<const uint8_t *>(d.addrw)[(size_t)m * 24u + k];
}

// the highest present members, descending, as far as `want` (at most 3) goes; returns how many were found
__device__ inline uint32_t ringcs_highest(const unsigned long long *bm, uint32_t ngroups, uint32_t want, uint32_t *out) {
    uint32_t found = 0;
    for (uint32_t g = ngroups; g-- > 0 && found < want;) {
        const unsigned long long b0 = bm[g * 4u], b1 = bm[g * 4u + 1], b2 = bm[g * 4u + 2], b3 = bm[g * 4u + 3];
        unsigned long long any = b0 | b1 | b2 | b3;
        while (any && found < want) {
            const uint32_t l = 63u - (uint32_t)__builtin_clzll(any);
            any &= ~(1ull << l);
            const uint32_t m = g * ROUTE_GROUP + l * 4u;
            if (((b3 >> l) & 1ull) && found < want) out[found++] = m + 3;
            if (((b2 >> l) & 1ull) && found < want) out[found++] = m + 2;
            if (((b1 >> l) & 1ull) && found < want) out[found++] = m + 1;
            if (((b0 >> l) & 1ull) && found < want) out[found++] = m;
        }
    }
    return found;
}

// grid = requested rows, RINGCS_THREADS threads, dynamic LDS route_bitmap_bytes(NP)
__global__ void __launch_bounds__(RINGCS_THREADS) k_ringcs_scan(DS d, const uint32_t *rows, unsigned long long *keys,
                                                                 uint32_t *cnts) {
    extern __shared__ unsigned long long route_bm[];
    __shared__ uint32_t wcnt[RINGCS_THREADS / 64];
    __shared__ unsigned long long wkey[RINGCS_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t row = rows[blockIdx.x];
    if (row >= d.NL) return;                                           // (the whole workgroup, before any barrier)
    const uint32_t cnt = route_stage_bitmap(d, row, route_bm, wcnt);
    unsigned long long key = 0;
    for (uint32_t m = tid; m < d.N; m += RINGCS_THREADS)
        if (route_present(route_bm, m)) key += ringcs_mix(m);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) key += (unsigned long long)__shfl_xor((long long)key, s);
    if (lane == 0) wkey[wave] = key;
    __syncthreads();
    if (tid == 0) {
        keys[blockIdx.x] = wkey[0] + wkey[1] + wkey[2] + wkey[3];
        cnts[blockIdx.x] = cnt;
    }
}

// grid = requested rows. rep[j] = the position (in rows) of row j's representative; differ[j] (zeroed by the host) is
// set when the two rows do not hold the same members alive or suspect
__global__ void __launch_bounds__(RINGCS_THREADS) k_ringcs_verify(DS d, const uint32_t *rows, const uint32_t *rep, uint32_t n,
                                                                   uint32_t *differ) {
    const uint32_t j = blockIdx.x, r = rep[j];
    if (r == j || r >= n) return;
    const uint32_t ra = rows[j], rb = rows[r];
    if (ra == rb || ra >= d.NL || rb >= d.NL) return;
    const uint32_t *pa = d.mw + (size_t)ra * d.NP, *pb = d.mw + (size_t)rb * d.NP;
    bool diff = false;
    for (uint32_t c0 = threadIdx.x * 4u; c0 < d.NP; c0 += RINGCS_THREADS * 4u) {   // NP is a multiple of 64: c0 < NP covers c0 + 3
        const uint4 a = *reinterpret_cast<const uint4 *>(pa + c0), b = *reinterpret_cast<const uint4 *>(pb + c0);
        diff |= c0 < d.N && ((a.x & 7u) <= ST_SUSPECT) != ((b.x & 7u) <= ST_SUSPECT);
        diff |= c0 + 1 < d.N && ((a.y & 7u) <= ST_SUSPECT) != ((b.y & 7u) <= ST_SUSPECT);
        diff |= c0 + 2 < d.N && ((a.z & 7u) <= ST_SUSPECT) != ((b.z & 7u) <= ST_SUSPECT);
        diff |= c0 + 3 < d.N && ((a.w & 7u) <= ST_SUSPECT) != ((b.w & 7u) <= ST_SUSPECT);
    }
    if (diff) differ[j] = 1u;
}

// premix block b of the string (bytes 20 b .. 20 b + 32 of the byte ring) into slot i of a premix buffer
__device__ __forceinline__ void ringcs_premix(const uint32_t *sring, uint32_t b, uint32_t iters, uint2 *slot) {
    uint32_t w[8];
    uint32_t at = (5u * b) % RINGCS_RBW;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        w[i] = sring[at];
        at = at + 1 == RINGCS_RBW ? 0u : at + 1;
    }
    const bool last = b + 1 >= iters;
    const uint32_t an = last ? 0u : w[5], bn = last ? 0u : w[6], cn = last ? 0u : w[7];
    constexpr uint32_t C = 0xe6546b64u;
    const uint32_t ad = w[0] + w[3];
    slot[0] = make_uint2(fh_m(w[2]), 3u * C + w[0] + ad + bn);                   // g: M(c), 3C + 2a + d + b'
    slot[1] = make_uint2(fh_m(w[1] + w[4] * FH_C1), 2u * C + ad + cn);           // f: M(b + e c1), 2C + a + d + c'
    slot[2] = make_uint2(fh_m(w[3]), C + w[4] + an);                             // h: M(d), C + e + a'
    slot[3] = make_uint2(0u, 0u);
}

// grid = representatives, RINGCS_THREADS threads, dynamic LDS route_bitmap_bytes(NP).
// hlist[b] = the position (in rows) of representative b; csr[position] receives its checksum
__global__ void __launch_bounds__(RINGCS_THREADS) k_ringcs_hash(DS d, const uint32_t *rows, const uint32_t *hlist, uint32_t *csr) {
    extern __shared__ unsigned long long route_bm[];
    __shared__ uint32_t sring[RINGCS_RBW];
    __shared__ uint2 mring[2][RINGCS_NB * 4];
    __shared__ uint32_t wcnt[RINGCS_THREADS / 64];
    __shared__ uint32_t xin[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t pos = hlist[blockIdx.x];
    const uint32_t row = rows[pos];
    if (row >= d.NL) return;                                           // (the whole workgroup, before any barrier)
    const uint32_t cnt = route_stage_bitmap(d, row, route_bm, wcnt);
    const uint32_t ngroups = route_groups(d.NP);
    const uint32_t W = d.W, RL = W + 1u;
    if (cnt <= 1) {                                                    // the empty string, or one address: no chain
        if (tid == 0) {
            uint8_t buf[28];
            uint32_t m = 0;
            const uint32_t have = ringcs_highest(route_bm, ngroups, cnt, &m);
            for (uint32_t k = 0; k < 28; k++) buf[k] = have && k < W ? (uint8_t)ringcs_addr_byte(d, m, k) : (uint8_t)0;
            csr[pos] = fp32_dev(buf, have ? W : 0u);
        }
        return;
    }
    const uint32_t len = cnt * RL - 1u, iters = (len - 1u) / 20u;      // len >= 27: the block chain
    if (tid == RINGCS_THREADS - 1) {                                   // FH::init from the last 20 bytes of S
        uint32_t hi[3] = {0, 0, 0};
        (void)ringcs_highest(route_bm, ngroups, 3u, hi);               // cnt >= 2: two records cover 20 bytes (W >= 13)
        uint32_t t[5] = {0, 0, 0, 0, 0};
        for (uint32_t q = 0; q < 20; q++) {
            const uint32_t p = len - 20u + q, r = p / RL, k = p - r * RL, back = cnt - 1u - r;
            const uint32_t byte = k == W ? (uint32_t)';' : ringcs_addr_byte(d, hi[back < 3 ? back : 2], k);
            t[q >> 2] |= byte << (8u * (q & 3u));
        }
        FH fh;
        fh.init(len, t[0], t[1], t[2], t[3], t[4]);
        xin[0] = fh.g; xin[1] = fh.f; xin[2] = fh.h; xin[3] = 0u;
    }
    uint8_t *s8 = reinterpret_cast<uint8_t *>(sring);
    const uint32_t nchunks = (d.N + RINGCS_CHUNK - 1) / RINGCS_CHUNK;
    const uint32_t sh = tid == 0 ? 1u : 0u;
    uint32_t X = 0;                                                    // the chain lanes' carried value
    uint32_t recs = 0, bdone = 0;                                      // records in the ring so far, blocks chained
    for (uint32_t c = 0; c < nchunks; c++) {
        // ---- expand the chunk: its present members' records, at their string positions ----
        uint32_t before = 0, total = 0;                                // present members of the chunk below my group, all
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            const uint32_t g = c * 4u + q;
            const uint32_t pc = g < ngroups ? (uint32_t)(__popcll(route_bm[g * 4u]) + __popcll(route_bm[g * 4u + 1]) +
                                                         __popcll(route_bm[g * 4u + 2]) + __popcll(route_bm[g * 4u + 3]))
                                            : 0u;
            before += q < wave ? pc : 0u;
            total += pc;
        }
        const uint32_t g = c * 4u + wave;
        if (g < ngroups && total) {
            const unsigned long long b[4] = {route_bm[g * 4u], route_bm[g * 4u + 1], route_bm[g * 4u + 2], route_bm[g * 4u + 3]};
            const unsigned long long below = (1ull << lane) - 1ull;
            uint32_t rec = recs + before + (uint32_t)(__popcll(b[0] & below) + __popcll(b[1] & below) + __popcll(b[2] & below) +
                                                      __popcll(b[3] & below));
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                if (!((b[j] >> lane) & 1ull)) continue;
                const uint32_t m = g * ROUTE_GROUP + lane * 4u + j;    // present: m < N
                const uint2 *ap = reinterpret_cast<const uint2 *>(d.addrw + (size_t)m * 6u);
                const uint2 a0 = ap[0], a1 = ap[1], a2 = ap[2];
                const uint32_t aw[6] = {a0.x, a0.y, a1.x, a1.y, a2.x, a2.y};
                uint32_t p = (rec * RL) % RINGCS_RB;
#pragma unroll
                for (uint32_t k = 0; k < 20; k++) {
                    if (k < W) {
                        s8[p] = (uint8_t)(aw[k >> 2] >> (8u * (k & 3u)));
                        p = p + 1 == RINGCS_RB ? 0u : p + 1;
                    }
                }
                if (rec + 1 < cnt) s8[p] = (uint8_t)';';
                rec++;
            }
        }
        recs += total;
        __syncthreads();
        // ---- the blocks that are ready: premix in batches, double buffered against the chain ----
        const bool complete = recs >= cnt;
        const uint32_t have = recs * RL;
        const uint32_t lim = complete ? iters : min(iters, have >= RINGCS_HOLD ? (have - RINGCS_HOLD) / 20u + 1u : 0u);
        const uint32_t nblk = lim > bdone ? lim - bdone : 0u;
        const uint32_t nb = (nblk + RINGCS_NB - 1) / RINGCS_NB;
        if (nb) {
            if (wave >= 1 && tid - 64u < min(RINGCS_NB, nblk)) ringcs_premix(sring, bdone + tid - 64u, iters, &mring[0][(tid - 64u) * 4u]);
            __syncthreads();
        }
        for (uint32_t k = 0; k < nb; k++) {
            const uint32_t b0 = bdone + k * RINGCS_NB, n = min(RINGCS_NB, lim - b0);
            if (wave == 0) {
                if (tid < 4) {
                    if (b0 == 0) X = tid == 3 ? 0u : xin[tid] + sring[tid == 0 ? 1 : tid == 1 ? 2 : 0];   // g + b, f + c, h + a
                    const uint2 *mp = &mring[k & 1u][tid];
                    uint32_t j = 0;
                    for (; j + 8 <= n; j += 8) {
                        uint2 v[8];
#pragma unroll
                        for (uint32_t u = 0; u < 8; u++) v[u] = mp[(j + u) * 4u];
#pragma unroll
                        for (uint32_t u = 0; u < 8; u++) fh_quad_step(X, v[u].x, v[u].y, sh);
                    }
                    for (; j < n; j++) {
                        const uint2 v = mp[j * 4u];
                        fh_quad_step(X, v.x, v.y, sh);
                    }
                }
            } else if (k + 1 < nb) {
                const uint32_t b1 = b0 + RINGCS_NB, n1 = min(RINGCS_NB, lim - b1);
                if (tid - 64u < n1) ringcs_premix(sring, b1 + tid - 64u, iters, &mring[(k + 1) & 1u][(tid - 64u) * 4u]);
            }
            __syncthreads();
        }
        bdone = lim;
        if (complete) break;                                           // (cnt is the same in every thread)
    }
    if (tid < 4) {                                                     // the last block's look-ahead is zero: X = g, f, h
        const uint32_t g = (uint32_t)__shfl((int)X, 0), f = (uint32_t)__shfl((int)X, 1), hh = (uint32_t)__shfl((int)X, 2);
        if (tid == 0) {
            FH fh{hh, g, f};
            csr[pos] = fh.fin();
        }
    }
}

// one lane per requested row: its representative's checksum
__global__ void __launch_bounds__(256) k_ringcs_scatter(const uint32_t *rep, const uint32_t *csr, uint32_t n, uint32_t *out) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < n) out[j] = csr[rep[j] < n ? rep[j] : j];
}

}  // namespace swimdev
