// swimsim_census.hip — member census: how the observer rows of this handle hold each member.
//
// Column reductions over the dense row words mw[NL][NP], which are always current (hot columns write both copies,
// DESIGN.md §3). Per member: the number of counted rows holding it in each status (alive, suspect, faulty, leave,
// tombstone, unknown = status 7) and the smallest and largest incarnation step e over the rows that know it. The
// kernels only read engine state; nothing on the side streams writes mw, so main-stream order is enough.
//
//   k_census       every column: a wave streams 256 columns (one dwordx4 per lane) down a chunk of rows and writes one
//                  partial slab per chunk; k_census_sum adds the slabs per column (store-and-sum: no atomics on the
//                  data, the result does not depend on arrival order).
//   k_census_cols  n listed columns (short lists, and the per-round trace inside swimsim_step): one wave per chunk of
//                  rows, lane = listed column, one 64-B sector per row and column. The wave that takes the last ticket
//                  adds the chunks' partials in chunk order and writes the result, so one launch does it all.
#pragma once
#include "swimsim_device.h"

namespace swimdev {

// A lane keeps the six status counters of a column in one 64-bit accumulator, 10 bits each: a chunk may hold at most
// 2^10 - 1 = 1,023 rows. Both chunk sizes below stay under that bound.
constexpr uint32_t CENSUS_FIELD_BITS = 10;
constexpr uint32_t CENSUS_FIELD_MASK = (1u << CENSUS_FIELD_BITS) - 1u;
constexpr uint32_t CENSUS_CHUNK_ROWS = 512;        // rows per partial slab of k_census
constexpr uint32_t CENSUS_COLS_CHUNK_ROWS = 256;   // rows per wave of k_census_cols
static_assert(CENSUS_CHUNK_ROWS <= CENSUS_FIELD_MASK && CENSUS_COLS_CHUNK_ROWS <= CENSUS_FIELD_MASK,
              "a packed status counter must hold a whole chunk of rows");
constexpr uint32_t CENSUS_WAVE_COLS = 256;         // columns per wave of k_census (64 lanes x dwordx4)
constexpr uint32_t CENSUS_BLOCK_COLS = 1024;       // columns per workgroup (4 waves)
constexpr uint32_t CENSUS_UNROLL = 8;              // rows in flight per wave
// A listed column costs one 64-B sector per row, a streamed one 4 B: a list of n members takes k_census_cols while
// n * CENSUS_LIST_WORDS <= NP (its sector traffic is at most the full census's row traffic), k_census beyond.
constexpr uint32_t CENSUS_LIST_WORDS = 16;
constexpr uint32_t CENSUS_NFIELDS = 8;             // per column: six counts, min e (0xFFFFFFFF: none), max e + 1 (0: none)
constexpr uint32_t CENSUS_TRACE_MAX = 64;          // tracked members of a trace

struct CensusAcc {
    unsigned long long c;
    uint32_t mn, mx;
};
__device__ __forceinline__ CensusAcc census_zero() { return CensusAcc{0ull, 0xFFFFFFFFu, 0u}; }
__device__ __forceinline__ void census_add(CensusAcc &a, uint32_t w) {
    const uint32_t s = w & 7u, f = s < 5u ? s : 5u, e = w >> 3;
    a.c += 1ull << (f * CENSUS_FIELD_BITS);
    a.mn = min(a.mn, s < 5u ? e : 0xFFFFFFFFu);
    a.mx = max(a.mx, s < 5u ? e + 1u : 0u);
}
__device__ __forceinline__ uint32_t census_count(const CensusAcc &a, uint32_t f) {
    return (uint32_t)(a.c >> (f * CENSUS_FIELD_BITS)) & CENSUS_FIELD_MASK;
}

// rows [g0, g0 + 64) of the chunk ending at r1 that count: bit b = row g0 + b (wave-uniform)
__device__ __forceinline__ unsigned long long census_rows(const DS &d, uint32_t g0, uint32_t r1, uint32_t all) {
    const uint32_t rr = g0 + lane_id();
    return __ballot(rr < r1 && (all || d.live[d.lo + rr]));
}

// grid (ceil(NP / CENSUS_BLOCK_COLS), ceil(NL / CENSUS_CHUNK_ROWS)), 256 threads.
// slab[chunk][field][NP]: the partial of every column over the chunk's counted rows.
__global__ void __launch_bounds__(256) k_census(DS d, uint32_t all, uint32_t *slab) {
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const uint32_t cw = blockIdx.x * CENSUS_BLOCK_COLS + wave * CENSUS_WAVE_COLS;
    if (cw >= d.NP) return;                                        // (the whole wave)
    const uint32_t c0 = cw + lane * 4;
    const bool act = c0 < d.NP;                                    // NP is a multiple of 64: c0 + 3 < NP as well
    const uint32_t chunk = blockIdx.y;
    const uint32_t r0 = chunk * CENSUS_CHUNK_ROWS, r1 = min(r0 + CENSUS_CHUNK_ROWS, d.NL);
    CensusAcc a0 = census_zero(), a1 = census_zero(), a2 = census_zero(), a3 = census_zero();
    const uint32_t *base = d.mw + (act ? c0 : 0u);
    for (uint32_t g0 = r0; g0 < r1; g0 += 64) {
        const unsigned long long rows = census_rows(d, g0, r1, all);
        for (uint32_t b = 0; b < 64; b += CENSUS_UNROLL) {
            const uint32_t m = (uint32_t)(rows >> b) & ((1u << CENSUS_UNROLL) - 1u);
            if (!m) continue;
            uint4 w[CENSUS_UNROLL];
#pragma unroll
            for (uint32_t k = 0; k < CENSUS_UNROLL; k++)
                if ((m >> k) & 1u) w[k] = *reinterpret_cast<const uint4 *>(base + (size_t)(g0 + b + k) * d.NP);
#pragma unroll
            for (uint32_t k = 0; k < CENSUS_UNROLL; k++)
                if ((m >> k) & 1u) {
                    census_add(a0, w[k].x);
                    census_add(a1, w[k].y);
                    census_add(a2, w[k].z);
                    census_add(a3, w[k].w);
                }
        }
    }
    if (!act) return;
    uint32_t *out = slab + (size_t)chunk * CENSUS_NFIELDS * d.NP + c0;
#pragma unroll
    for (uint32_t f = 0; f < 6; f++)
        *reinterpret_cast<uint4 *>(out + (size_t)f * d.NP) =
            make_uint4(census_count(a0, f), census_count(a1, f), census_count(a2, f), census_count(a3, f));
    *reinterpret_cast<uint4 *>(out + (size_t)6 * d.NP) = make_uint4(a0.mn, a1.mn, a2.mn, a3.mn);
    *reinterpret_cast<uint4 *>(out + (size_t)7 * d.NP) = make_uint4(a0.mx, a1.mx, a2.mx, a3.mx);
}

// one thread per reported column (cols[i], or i when cols is null): the slabs added in chunk order, res[i][8]
__global__ void __launch_bounds__(256) k_census_sum(const uint32_t *slab, uint32_t nchunks, uint32_t NP, const uint32_t *cols,
                                                    uint32_t n, uint32_t *res) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = cols ? cols[i] : i;
    uint32_t v[CENSUS_NFIELDS] = {0, 0, 0, 0, 0, 0, 0xFFFFFFFFu, 0};
    for (uint32_t ch = 0; ch < nchunks; ch++) {
        const uint32_t *p = slab + (size_t)ch * CENSUS_NFIELDS * NP + c;
#pragma unroll
        for (uint32_t f = 0; f < 6; f++) v[f] += p[(size_t)f * NP];
        v[6] = min(v[6], p[(size_t)6 * NP]);
        v[7] = max(v[7], p[(size_t)7 * NP]);
    }
    uint4 *o = reinterpret_cast<uint4 *>(res + (size_t)i * CENSUS_NFIELDS);
    o[0] = make_uint4(v[0], v[1], v[2], v[3]);
    o[1] = make_uint4(v[4], v[5], v[6], v[7]);
}

// grid ceil(NL / CENSUS_COLS_CHUNK_ROWS) (at least 1), 64 threads. part[chunk][n][8] and nlp[chunk] (counted rows of the
// chunk) are the partials; *ticket is 0 between launches. The last wave writes, per listed column j, nf fields at
// dst[j * nf]. Census: dst = out. Trace (tstate = {cursor, dropped}): dst = the record at the device cursor, out +
// cursor * recwords, headed by {round, counted rows}; with tcap records held the round is counted as dropped instead.
__global__ void __launch_bounds__(64) k_census_cols(DS d, const uint32_t *cols, uint32_t n, uint32_t all, uint32_t *part,
                                                    uint32_t *nlp, uint32_t *ticket, uint32_t *out, uint32_t nf,
                                                    uint32_t *tstate, uint32_t tcap, uint32_t recwords, uint32_t round) {
    const uint32_t lane = lane_id(), chunk = blockIdx.x, nchunks = gridDim.x;
    const uint32_t r0 = chunk * CENSUS_COLS_CHUNK_ROWS, r1 = min(r0 + CENSUS_COLS_CHUNK_ROWS, d.NL);
    for (uint32_t j0 = 0; j0 < n; j0 += 64) {                      // (one pass over the rows per 64 listed columns)
        const uint32_t j = j0 + lane;
        const bool act = j < n;
        const uint32_t *base = d.mw + (act ? cols[j] : 0u);
        CensusAcc a = census_zero();
        uint32_t counted = 0;
        for (uint32_t g0 = r0; g0 < r1; g0 += 64) {
            const unsigned long long rows = census_rows(d, g0, r1, all);
            counted += (uint32_t)__popcll(rows);
            for (uint32_t b = 0; b < 64; b += CENSUS_UNROLL) {
                const uint32_t m = (uint32_t)(rows >> b) & ((1u << CENSUS_UNROLL) - 1u);
                if (!m) continue;
                uint32_t w[CENSUS_UNROLL];
#pragma unroll
                for (uint32_t k = 0; k < CENSUS_UNROLL; k++)
                    if ((m >> k) & 1u) w[k] = base[(size_t)(g0 + b + k) * d.NP];
#pragma unroll
                for (uint32_t k = 0; k < CENSUS_UNROLL; k++)
                    if ((m >> k) & 1u) census_add(a, w[k]);
            }
        }
        if (act) {
            uint4 *o = reinterpret_cast<uint4 *>(part + ((size_t)chunk * n + j) * CENSUS_NFIELDS);
            o[0] = make_uint4(census_count(a, 0), census_count(a, 1), census_count(a, 2), census_count(a, 3));
            o[1] = make_uint4(census_count(a, 4), census_count(a, 5), a.mn, a.mx);
        }
        if (j0 == 0 && lane == 0) nlp[chunk] = counted;
    }
    // the last wave to finish adds the partials (threadfence reduction: release, ticket, acquire)
    __threadfence();
    uint32_t t = 0;
    if (lane == 0) t = atomicAdd(ticket, 1u);
    t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
    if (t != nchunks - 1) return;
    __threadfence();
    if (lane == 0) *ticket = 0;
    uint32_t *dst = out;
    if (tstate) {
        const uint32_t cur = tstate[0];
        if (cur >= tcap) {
            if (lane == 0) tstate[1] += 1;
            return;
        }
        uint32_t nl = 0;
        for (uint32_t ch = lane; ch < nchunks; ch += 64) nl += nlp[ch];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) nl += __shfl_xor(nl, off, 64);
        dst = out + (size_t)cur * recwords;
        if (lane == 0) {
            dst[0] = round;
            dst[1] = nl;
            tstate[0] = cur + 1;
        }
        dst += 2;
    }
    for (uint32_t j = lane; j < n; j += 64) {
        uint32_t v[CENSUS_NFIELDS] = {0, 0, 0, 0, 0, 0, 0xFFFFFFFFu, 0};
        for (uint32_t ch = 0; ch < nchunks; ch++) {
            const uint4 *p = reinterpret_cast<const uint4 *>(part + ((size_t)ch * n + j) * CENSUS_NFIELDS);
            const uint4 x = p[0], y = p[1];
            v[0] += x.x; v[1] += x.y; v[2] += x.z; v[3] += x.w;
            v[4] += y.x; v[5] += y.y;
            v[6] = min(v[6], y.z);
            v[7] = max(v[7], y.w);
        }
        for (uint32_t f = 0; f < nf; f++) dst[(size_t)j * nf + f] = v[f];
    }
}

}  // namespace swimdev
