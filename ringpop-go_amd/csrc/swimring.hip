// swimring.hip — the consistent-hash ring Ringpop feeds from swim's applied changes
// (include/swimring.h states the semantics and the reference lines).
//
// HBM layout: the ring is one ascending array of u64 points (hash << 32 | server id); hashes are
// unique in it (a collision keeps the first inserter, rbtree.go:122-126). Server names live in a
// device byte pool (offset, length per id). An AddRemoveServers batch runs as:
//   k_ring_points   one lane per (added server, replica): Fingerprint32(name ‖ decimal(i)),
//                   key = hash << 32 | batch sequence (insertion order: server order, then i)
//   radix sort      by (hash, sequence)
//   k_ring_keep     keep the first point of each hash that the ring does not already hold
//   select + sort   append the kept points to the ring, sort the u64 points
//   k_ring_points   replica hashes of the removed servers (hash only), radix sort
//   k_ring_drop     drop every ring point whose hash is one of them (rbtree Delete by value)
// Lookups: one lane per key hashes it and binary-searches the ring (lower bound, wrap to 0).
// LookupN for a batch: one wave per key walks the ring 64 points per step (k_ring_lookup_n_batch); groupReplicas
// inverts the owner matrix with a radix sort of (owner << 32 | key index) and a boundary pass.
#include "../../include/swimring.h"
#include "../../include/swimsim.h"
#include "swimsim_device.h"
#include "swimsim_hash.h"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

using namespace swimdev;

namespace {

constexpr uint32_t RING_NAME_MAX = 240;     // longest server name a replica string is built from
constexpr uint32_t RING_STR_MAX = RING_NAME_MAX + 10;

// one lane per (server of the batch, replica): keys[j] = hash << 32 | j, vals[j] = server id
__global__ void k_ring_points(const uint8_t *names, const uint64_t *noff, const uint32_t *nlen, const int32_t *ids,
                              uint32_t nsrv, uint32_t R, unsigned long long *keys, uint32_t *vals) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nsrv * R) return;
    const uint32_t k = j / R, i = j - k * R;
    const int32_t id = ids[k];
    uint8_t buf[RING_STR_MAX + 4];
    const uint32_t len = replica_string(names + noff[id], nlen[id], i, buf);
    buf[len] = buf[len + 1] = buf[len + 2] = buf[len + 3] = 0;
    keys[j] = ((unsigned long long)fp32_dev(buf, len) << 32) | j;
    vals[j] = (uint32_t)id;
}

__device__ __forceinline__ bool ring_has(const unsigned long long *ring, uint32_t P, uint32_t h) {
    const uint32_t p = lower_bound_u64(ring, P, (unsigned long long)h << 32);
    return p < P && (uint32_t)(ring[p] >> 32) == h;
}

// sorted new points: keep the first of each hash unless the ring already has it; out = hash << 32 | id
__global__ void k_ring_keep(const unsigned long long *skeys, const uint32_t *svals, uint32_t n,
                            const unsigned long long *ring, uint32_t P, uint8_t *flag, unsigned long long *out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t h = (uint32_t)(skeys[j] >> 32);
    const bool first = j == 0 || (uint32_t)(skeys[j - 1] >> 32) != h;
    flag[j] = first && !ring_has(ring, P, h) ? 1 : 0;
    out[j] = ((unsigned long long)h << 32) | svals[j];
}

// ring points whose hash is a removed server's replica hash are dropped (sorted delete keys)
__global__ void k_ring_drop(const unsigned long long *ring, uint32_t P, const unsigned long long *dkeys, uint32_t nd,
                            uint8_t *flag) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const uint32_t h = (uint32_t)(ring[p] >> 32);
    const uint32_t q = lower_bound_u64(dkeys, nd, (unsigned long long)h << 32);
    flag[p] = (q < nd && (uint32_t)(dkeys[q] >> 32) == h) ? 0 : 1;
}

__global__ void k_fp32_batch(const uint8_t *bytes, const uint64_t *off, uint32_t n, uint32_t *out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t a = off[k], len = off[k + 1] - a;
    out[k] = fp32_dev(bytes + a, (uint32_t)len);                  // the ld32 tail reads stay inside the
}                                                                 // padded byte buffer

// Lookup: owner of the first point >= Fingerprint32(key), wrapping to the first point
__global__ void k_ring_lookup(const uint8_t *bytes, const uint64_t *off, uint32_t n, const unsigned long long *ring,
                              uint32_t P, int32_t *out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    if (P == 0) { out[k] = -1; return; }
    const uint64_t a = off[k];
    const uint32_t h = fp32_dev(bytes + a, (uint32_t)(off[k + 1] - a));
    uint32_t p = lower_bound_u64(ring, P, (unsigned long long)h << 32);
    if (p == P) p = 0;
    out[k] = (int32_t)(uint32_t)ring[p];
}

// LookupN: distinct owners walking up from the key's hash, then from 0 (rbtree.go:262-286). One workgroup:
// its threads clear a seen-bitmap over server ids, then one lane walks the ring (O(P) at worst, one bit test
// per point; the order of first occurrences decides which n owners are taken)
__global__ void k_ring_lookup_n(const uint8_t *key, uint32_t len, const unsigned long long *ring, uint32_t P, uint32_t n,
                                int32_t *out, uint32_t *nout, uint32_t *seen, uint32_t seen_words) {
    if (blockIdx.x) return;
    for (uint32_t i = threadIdx.x; i < seen_words; i += blockDim.x) seen[i] = 0;
    __syncthreads();
    if (threadIdx.x) return;
    uint32_t got = 0;
    const uint32_t h = fp32_dev(key, len);
    const uint32_t start = lower_bound_u64(ring, P, (unsigned long long)h << 32);
    for (int pass = 0; pass < 2 && got < n; pass++) {
        for (uint32_t p = pass ? 0 : start; p < P && got < n; p++) {
            const uint32_t o = (uint32_t)ring[p];
            const uint32_t bit = 1u << (o & 31);
            if (seen[o >> 5] & bit) continue;
            seen[o >> 5] |= bit;
            out[got++] = (int32_t)o;
        }
    }
    *nout = got;
}

// ---------------------------------------------------------------------------------------------
// LookupN for a batch of keys: one wave per key, LN_WAVES keys in flight per workgroup. Every lane hashes the
// key (wave-uniform addresses, so the hash is scalar) and the wave finds the lower bound together
// (wave_lower_bound_u64); then it loads 64 consecutive points per step (index modulo P, at most P points in
// all). A lane's owner is a candidate if it is not among the owners taken so far:
//   n <= LN_LIST_MAX  the taken owners are a list in LDS (at most n - 1 broadcast reads per step);
//   n >  LN_LIST_MAX  they are a bitmap over server ids, one slice per wave of the grid in device scratch,
//                     zero at entry and cleared again bit by bit when the key is done (BITMAP).
// Candidates that repeat a lower lane's owner are dropped without touching memory: the lowest candidate's owner
// is read with readlane, one ballot finds every lane holding it, and the loop ends once n - got distinct
// owners are found. The popcount of the new lanes below a lane is its output slot.
// The wave's lanes read what other lanes of the same wave wrote one step earlier (list, bitmap, output row):
// those accesses are atomic loads / stores with a wavefront-scope fence between the steps.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t LN_WAVES = 4;
constexpr uint32_t LN_LIST_MAX = 16;
constexpr uint32_t LN_MAX_WAVES = 8192;                           // bitmap mode: 256 CUs x 32 waves
constexpr size_t LN_SEEN_BYTES = (size_t)64 << 20;                // bitmap mode: scratch budget for the slices

__device__ __forceinline__ uint32_t ld_lanes(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_lanes(uint32_t *p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void fence_lanes() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lower_bound_u64 by a whole wave: each step the lanes probe up to 64 evenly spaced points of the remaining range
// and one ballot keeps the gap the bound lies in, so a ring of P points takes log65 P dependent loads, not log2 P
__device__ __forceinline__ uint32_t wave_lower_bound_u64(const unsigned long long *a, uint32_t n, unsigned long long x,
                                                         uint32_t lane) {
    uint64_t lo = 0, hi = n;                                      // a[i] < x below lo, a[i] >= x from hi on
    while (lo < hi) {
        const uint64_t step = (hi - lo + 63) / 64;
        const uint64_t i = lo + lane * step;
        const uint32_t c = (uint32_t)__popcll(__ballot(i < hi && a[i] < x));   // sorted: a prefix of the probes
        if (c == 0) break;                                        // a[lo] >= x
        if (lo + c * step < hi) hi = lo + c * step;               // probe c, if there is one, is >= x
        lo += (c - 1) * step + 1;                                 // probe c - 1 is < x
    }
    return (uint32_t)lo;
}

template <bool BITMAP>
__global__ __launch_bounds__(LN_WAVES * 64) void k_ring_lookup_n_batch(
    const uint8_t *bytes, const uint64_t *off, uint32_t nkeys, const unsigned long long *ring, uint32_t P, uint32_t n,
    int32_t *out, uint32_t *cnt, uint32_t *seen, uint32_t seen_words) {
    __shared__ uint32_t taken[LN_WAVES][LN_LIST_MAX];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t wave = blockIdx.x * LN_WAVES + w, nwaves = gridDim.x * LN_WAVES;
    uint32_t *bits = BITMAP ? seen + (size_t)wave * seen_words : nullptr;
    const unsigned long long below = (1ull << lane) - 1;
    for (uint64_t k = wave; k < nkeys; k += nwaves) {
        const uint64_t a = off[k];
        const uint32_t h = __builtin_amdgcn_readfirstlane(fp32_dev(bytes + a, (uint32_t)(off[k + 1] - a)));
        uint32_t start = __builtin_amdgcn_readfirstlane(wave_lower_bound_u64(ring, P, (unsigned long long)h << 32, lane));
        if (start == P) start = 0;
        uint32_t *row = (uint32_t *)out + k * n;
        uint32_t got = 0;
        for (uint64_t base = 0; base < P && got < n; base += 64) {
            const uint64_t idx = base + lane;
            const bool valid = idx < P;
            uint64_t p = start + idx;
            if (p >= P) p -= P;
            const uint32_t o = valid ? (uint32_t)ring[p] : 0;
            bool cand = valid;
            if (BITMAP) {
                if (valid) cand = !((ld_lanes(bits + (o >> 5)) >> (o & 31)) & 1);
            } else {
                for (uint32_t q = 0; q < got; q++) cand = cand && ld_lanes(&taken[w][q]) != o;
            }
            unsigned long long m = __ballot(cand), fresh = 0;
            const uint32_t need = n - got;
            uint32_t nf = 0;
            while (m && nf < need) {
                const uint32_t j = (uint32_t)__builtin_ctzll(m);
                const uint32_t oj = (uint32_t)__builtin_amdgcn_readlane((int)o, (int)j);
                fresh |= 1ull << j;
                nf++;
                m &= ~__ballot(cand && o == oj);                  // lane j and every repeat of its owner
            }
            if ((fresh >> lane) & 1) {
                const uint32_t slot = got + (uint32_t)__popcll(fresh & below);
                st_lanes(row + slot, o);
                if (BITMAP) atomicOr(bits + (o >> 5), 1u << (o & 31));
                else st_lanes(&taken[w][slot], o);                // slot < n <= LN_LIST_MAX
            }
            got += nf;
            fence_lanes();
        }
        if (BITMAP)                                               // leave the slice zero for the wave's next key
            for (uint32_t j = lane; j < got; j += 64) st_lanes(bits + (ld_lanes(row + j) >> 5), 0);
        for (uint32_t j = got + lane; j < n; j += 64) row[j] = 0xffffffffu;
        if (lane == 0) cnt[k] = got;
        fence_lanes();
    }
}

// n >= server count: every key's owners are every server, ascending id (lookupNNoLock's shortcut)
__global__ void k_ring_fill_all(const int32_t *all, uint32_t nall, uint32_t n, uint64_t total, int32_t *out,
                                uint32_t *cnt) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const uint32_t j = (uint32_t)(e % n);
    out[e] = j < nall ? all[j] : -1;
    if (j == 0) cnt[e / n] = nall;
}

// groupReplicas: entry e = (key k, column j) of the owner matrix becomes the sort key owner << 32 | k; the -1
// padding sorts behind every server
__global__ void k_group_keys(const int32_t *mat, uint32_t n, uint64_t total, unsigned long long *keys) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    keys[e] = ((unsigned long long)(uint32_t)mat[e] << 32) | (uint32_t)(e / n);
}

// sorted keys: key_idx[e] = the key index; the first entry of each destination (and of the padding) is
// flagged and carries destination << 32 | e
__global__ void k_group_bounds(const unsigned long long *skeys, uint64_t total, uint32_t *key_idx, uint8_t *flag,
                               unsigned long long *bound) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const uint32_t d = (uint32_t)(skeys[e] >> 32);
    key_idx[e] = (uint32_t)skeys[e];
    flag[e] = e == 0 || (uint32_t)(skeys[e - 1] >> 32) != d ? 1 : 0;
    bound[e] = ((unsigned long long)d << 32) | e;
}

uint32_t grid_for(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, (n + 255) / 256); }

}  // namespace

struct swimring {
    uint32_t R = 100;
    int device = 0;
    hipStream_t s = nullptr;
    std::string err;
    // server table (host) and its device copy
    std::unordered_map<std::string, int32_t> ids;
    std::vector<std::string> names;
    std::vector<uint8_t> in_set;
    uint32_t nset = 0;
    uint8_t *dnames = nullptr;
    uint64_t *dnoff = nullptr;
    uint32_t *dnlen = nullptr;
    size_t names_bytes_dev = 0, names_cap = 0, ids_cap = 0, ids_dev = 0;
    std::vector<uint64_t> hnoff;
    std::vector<uint32_t> hnlen;
    // ring
    unsigned long long *ring = nullptr, *ring2 = nullptr;
    uint32_t *seen = nullptr;                                     // LookupN's seen-bitmap over server ids
    size_t seen_cap = 0;
    uint32_t P = 0;
    size_t ring_cap = 0;
    uint32_t checksum = 0;
    // scratch
    unsigned long long *k0 = nullptr, *k1 = nullptr, *kept = nullptr;
    uint32_t *v0 = nullptr, *v1 = nullptr, *nsel = nullptr;
    uint8_t *flag = nullptr;
    int32_t *bid = nullptr;
    size_t scr_cap = 0, bid_cap = 0;
    void *cub = nullptr;
    size_t cub_cap = 0;
    uint8_t *bytes = nullptr;
    uint64_t *boff = nullptr;
    size_t bytes_cap = 0, boff_cap = 0;
    int32_t *iout = nullptr;
    uint32_t *uout = nullptr;
    size_t out_cap = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    double t_add = 0, t_look = 0;
    // LookupN batch / groupReplicas: owner matrix [nkeys x n] (its counts are uout), the waves' seen-bitmap slices
    int32_t *mat = nullptr;
    uint32_t *wseen = nullptr;
    size_t mat_cap = 0, wseen_cap = 0;
    double t_lookn = 0, t_group = 0;

    int fail(int code, const char *fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
};

#define RCHK(r, x)                                                                               \
    do {                                                                                         \
        hipError_t e_ = (x);                                                                     \
        if (e_ != hipSuccess) return (r)->fail(SWIMSIM_EHIP, "%s: %s", #x, hipGetErrorString(e_)); \
    } while (0)

namespace {

template <typename T>
int grow(swimring *r, T **p, size_t *cap, size_t need, bool keep = false, size_t keep_elems = 0) {
    if (need <= *cap) return 0;
    size_t c = std::max<size_t>(need + need / 2, 1024);
    T *q = nullptr;
    if (hipMalloc(&q, c * sizeof(T)) != hipSuccess) return r->fail(SWIMSIM_ENOMEM, "hipMalloc(%zu bytes)", c * sizeof(T));
    if (keep && *p && keep_elems)
        if (hipMemcpyAsync(q, *p, keep_elems * sizeof(T), hipMemcpyDeviceToDevice, r->s) != hipSuccess)
            return r->fail(SWIMSIM_EHIP, "ring copy");
    if (*p) {
        hipStreamSynchronize(r->s);
        hipFree(*p);
    }
    *p = q;
    *cap = c;
    return 0;
}

int intern(swimring *r, const char *s, int32_t *id) {
    auto it = r->ids.find(s);
    if (it != r->ids.end()) { *id = it->second; return 0; }
    const size_t len = strlen(s);
    if (len > RING_NAME_MAX) return r->fail(SWIMSIM_EINVAL, "server name longer than %u bytes", RING_NAME_MAX);
    *id = (int32_t)r->names.size();
    r->ids.emplace(s, *id);
    r->names.emplace_back(s);
    r->in_set.push_back(0);
    r->hnoff.push_back(r->hnoff.empty() ? 0 : r->hnoff.back() + r->hnlen.back());
    r->hnlen.push_back((uint32_t)len);
    return 0;
}

// upload server names interned since the last upload (append-only)
int sync_names(swimring *r) {
    const size_t n = r->names.size();
    if (n == r->ids_dev) return 0;
    const size_t total = r->hnoff.back() + r->hnlen.back();
    size_t cap = r->names_cap;
    if (int rc = grow(r, &r->dnames, &cap, total + 8, true, r->names_bytes_dev)) return rc;
    r->names_cap = cap;
    size_t icap = r->ids_cap, icap2 = r->ids_cap;
    if (int rc = grow(r, &r->dnoff, &icap, n, true, r->ids_dev)) return rc;
    if (int rc = grow(r, &r->dnlen, &icap2, n, true, r->ids_dev)) return rc;
    r->ids_cap = icap;
    std::string blob;
    for (size_t i = r->ids_dev; i < n; i++) blob += r->names[i];
    const size_t b0 = r->names_bytes_dev;
    if (!blob.empty()) RCHK(r, hipMemcpyAsync(r->dnames + b0, blob.data(), blob.size(), hipMemcpyHostToDevice, r->s));
    RCHK(r, hipMemcpyAsync(r->dnoff + r->ids_dev, r->hnoff.data() + r->ids_dev, (n - r->ids_dev) * 8, hipMemcpyHostToDevice, r->s));
    RCHK(r, hipMemcpyAsync(r->dnlen + r->ids_dev, r->hnlen.data() + r->ids_dev, (n - r->ids_dev) * 4, hipMemcpyHostToDevice, r->s));
    RCHK(r, hipStreamSynchronize(r->s));                         // the blob is a host temporary
    r->names_bytes_dev = total;
    r->ids_dev = n;
    return 0;
}

int ensure_scratch(swimring *r, size_t n) {
    size_t c;
    c = r->scr_cap; if (int rc = grow(r, &r->k0, &c, n)) return rc;
    c = r->scr_cap; if (int rc = grow(r, &r->k1, &c, n)) return rc;
    c = r->scr_cap; if (int rc = grow(r, &r->kept, &c, n)) return rc;
    c = r->scr_cap; if (int rc = grow(r, &r->v0, &c, n)) return rc;
    c = r->scr_cap; if (int rc = grow(r, &r->v1, &c, n)) return rc;
    c = r->scr_cap; if (int rc = grow(r, &r->flag, &c, n)) return rc;
    r->scr_cap = std::max(r->scr_cap, c);
    return 0;
}

int ensure_cub(swimring *r, size_t bytes) {
    size_t c = r->cub_cap;
    if (int rc = grow(r, (uint8_t **)&r->cub, &c, bytes)) return rc;
    r->cub_cap = c;
    return 0;
}

// replica points of the listed servers, sorted by (hash, insertion sequence) into k1 / v1
int hash_replicas(swimring *r, const std::vector<int32_t> &list) {
    const size_t n = list.size() * r->R;
    if (int rc = ensure_scratch(r, n)) return rc;
    size_t c = r->bid_cap;
    if (int rc = grow(r, &r->bid, &c, list.size())) return rc;
    r->bid_cap = c;
    RCHK(r, hipMemcpyAsync(r->bid, list.data(), list.size() * 4, hipMemcpyHostToDevice, r->s));
    hipLaunchKernelGGL(k_ring_points, dim3(grid_for(n)), dim3(256), 0, r->s, r->dnames, r->dnoff, r->dnlen, r->bid,
                       (uint32_t)list.size(), r->R, r->k0, r->v0);
    size_t tb = 0;
    hipcub::DeviceRadixSort::SortPairs(nullptr, tb, r->k0, r->k1, r->v0, r->v1, (int)n, 0, 64, r->s);
    if (int rc = ensure_cub(r, tb)) return rc;
    RCHK(r, hipcub::DeviceRadixSort::SortPairs(r->cub, tb, r->k0, r->k1, r->v0, r->v1, (int)n, 0, 64, r->s));
    RCHK(r, hipStreamSynchronize(r->s));                         // list is a host temporary
    return 0;
}

int upload_keys(swimring *r, const uint8_t *keys, const uint64_t *off, size_t nkeys) {
    const size_t nb = off[nkeys];
    size_t c = r->bytes_cap;
    if (int rc = grow(r, &r->bytes, &c, nb + 8)) return rc;
    r->bytes_cap = c;
    c = r->boff_cap;
    if (int rc = grow(r, &r->boff, &c, nkeys + 1)) return rc;
    r->boff_cap = c;
    c = r->out_cap;
    size_t c2 = r->out_cap;
    if (int rc = grow(r, &r->iout, &c, std::max<size_t>(nkeys, 64))) return rc;
    if (int rc = grow(r, &r->uout, &c2, std::max<size_t>(nkeys, 64))) return rc;
    r->out_cap = c;
    if (nb) RCHK(r, hipMemcpyAsync(r->bytes, keys, nb, hipMemcpyHostToDevice, r->s));
    RCHK(r, hipMemsetAsync(r->bytes + nb, 0, 8, r->s));
    RCHK(r, hipMemcpyAsync(r->boff, off, (nkeys + 1) * 8, hipMemcpyHostToDevice, r->s));
    return 0;
}

int compute_checksum(swimring *r) {
    std::vector<const std::string *> v;
    for (size_t i = 0; i < r->names.size(); i++)
        if (r->in_set[i]) v.push_back(&r->names[i]);
    std::sort(v.begin(), v.end(), [](const std::string *a, const std::string *b) { return *a < *b; });
    std::string joined;
    for (size_t i = 0; i < v.size(); i++) {
        if (i) joined += ';';
        joined += *v[i];
    }
    const uint64_t off[2] = {0, joined.size()};
    if (int rc = upload_keys(r, (const uint8_t *)joined.data(), off, 1)) return rc;
    hipLaunchKernelGGL(k_fp32_batch, dim3(1), dim3(64), 0, r->s, r->bytes, r->boff, 1u, r->uout);
    RCHK(r, hipMemcpyAsync(&r->checksum, r->uout, 4, hipMemcpyDeviceToHost, r->s));
    RCHK(r, hipStreamSynchronize(r->s));
    return 0;
}

// nkeys * n matrix entries are sort items (int) and CSR positions (u32)
bool replica_dims_ok(size_t nkeys, uint32_t n) {
    return nkeys <= 0x7fffffffu && (n == 0 || nkeys <= (size_t)0x7fffffffu / n);
}

// LookupN of nkeys keys (nkeys, n > 0) into r->mat [nkeys x n] and r->uout [nkeys]; both stay on the device
int lookup_n_device(swimring *r, const uint8_t *keys, const uint64_t *off, size_t nkeys, uint32_t n) {
    const size_t total = nkeys * n;
    size_t c = r->mat_cap;
    if (int rc = grow(r, &r->mat, &c, total)) return rc;
    r->mat_cap = c;
    if (int rc = upload_keys(r, keys, off, nkeys)) return rc;
    std::vector<int32_t> all;
    if (n >= r->nset) {                                           // lookupNNoLock: every server
        for (size_t i = 0; i < r->names.size(); i++)
            if (r->in_set[i]) all.push_back((int32_t)i);
        c = r->bid_cap;
        if (int rc = grow(r, &r->bid, &c, std::max<size_t>(all.size(), 1))) return rc;
        r->bid_cap = c;
        if (!all.empty()) RCHK(r, hipMemcpyAsync(r->bid, all.data(), all.size() * 4, hipMemcpyHostToDevice, r->s));
        RCHK(r, hipEventRecord(r->e0, r->s));
        hipLaunchKernelGGL(k_ring_fill_all, dim3(grid_for(total)), dim3(256), 0, r->s, r->bid, (uint32_t)all.size(), n,
                           (uint64_t)total, r->mat, r->uout);
    } else if (n <= LN_LIST_MAX) {
        RCHK(r, hipEventRecord(r->e0, r->s));
        hipLaunchKernelGGL(k_ring_lookup_n_batch<false>, dim3((uint32_t)((nkeys + LN_WAVES - 1) / LN_WAVES)),
                           dim3(LN_WAVES * 64), 0, r->s, r->bytes, r->boff, (uint32_t)nkeys, r->ring, r->P, n, r->mat,
                           r->uout, (uint32_t *)nullptr, 0u);
    } else {
        const size_t words = (r->names.size() + 31) / 32;
        const size_t waves = std::min<size_t>(std::max<size_t>(LN_SEEN_BYTES / (words * 4), LN_WAVES), LN_MAX_WAVES);
        const size_t blocks = std::min((nkeys + LN_WAVES - 1) / LN_WAVES, waves / LN_WAVES);
        c = r->wseen_cap;
        if (int rc = grow(r, &r->wseen, &c, blocks * LN_WAVES * words)) return rc;
        r->wseen_cap = c;
        RCHK(r, hipMemsetAsync(r->wseen, 0, blocks * LN_WAVES * words * 4, r->s));
        RCHK(r, hipEventRecord(r->e0, r->s));
        hipLaunchKernelGGL(k_ring_lookup_n_batch<true>, dim3((uint32_t)blocks), dim3(LN_WAVES * 64), 0, r->s, r->bytes,
                           r->boff, (uint32_t)nkeys, r->ring, r->P, n, r->mat, r->uout, r->wseen, (uint32_t)words);
    }
    RCHK(r, hipGetLastError());
    RCHK(r, hipEventRecord(r->e1, r->s));
    RCHK(r, hipStreamSynchronize(r->s));                         // all is a host temporary
    float ms = 0;
    hipEventElapsedTime(&ms, r->e0, r->e1);
    r->t_lookn = ms;
    return 0;
}

}  // namespace

extern "C" {

int swimring_create(uint32_t replica_points, int32_t device, swimring_t **out) {
    if (!out || replica_points == 0) return SWIMSIM_EINVAL;
    *out = nullptr;
    swimring *r = new swimring;
    r->R = replica_points;
    r->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&r->s, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&r->e0) != hipSuccess || hipEventCreate(&r->e1) != hipSuccess) {
        delete r;
        return SWIMSIM_EHIP;
    }
    *out = r;                                                     // checksum 0 until the first change (Go zero value)
    return SWIMSIM_OK;
}

int swimring_destroy(swimring_t *r) {
    if (!r) return SWIMSIM_OK;
    if (r->s) hipStreamSynchronize(r->s);
    void *bufs[] = {r->dnames, r->dnoff, r->dnlen, r->ring, r->ring2, r->k0, r->k1, r->kept, r->v0, r->v1, r->nsel,
                    r->flag, r->bid, r->cub, r->bytes, r->boff, r->iout, r->uout, r->seen, r->mat, r->wseen};
    for (void *p : bufs)
        if (p) hipFree(p);
    if (r->e0) hipEventDestroy(r->e0);
    if (r->e1) hipEventDestroy(r->e1);
    if (r->s) hipStreamDestroy(r->s);
    delete r;
    return SWIMSIM_OK;
}

const char *swimring_last_error(swimring_t *r) { return r ? r->err.c_str() : "null handle"; }

// the device half of AddRemoveServers: hash and insert the added servers' points, then drop the removed
// servers' points. *adds_done tells a failing caller whether the adds reached the ring
static int ring_apply(swimring *r, const std::vector<int32_t> &A, const std::vector<int32_t> &D, bool *adds_done) {
    RCHK(r, hipEventRecord(r->e0, r->s));
    size_t c;
    if (!A.empty()) {
        if (int rc = hash_replicas(r, A)) return rc;
        const uint32_t n = (uint32_t)(A.size() * r->R);
        hipLaunchKernelGGL(k_ring_keep, dim3(grid_for(n)), dim3(256), 0, r->s, r->k1, r->v1, n, r->ring, r->P, r->flag,
                           r->kept);
        c = r->ring_cap;
        const size_t need = (size_t)r->P + n;
        size_t c2 = r->ring_cap;
        if (int rc = grow(r, &r->ring, &c, need, true, r->P)) return rc;
        if (int rc = grow(r, &r->ring2, &c2, need)) return rc;
        r->ring_cap = std::min(c, c2);
        if (!r->nsel) RCHK(r, hipMalloc(&r->nsel, 16));
        size_t tb = 0;
        hipcub::DeviceSelect::Flagged(nullptr, tb, r->kept, r->flag, r->ring + r->P, r->nsel, (int)n, r->s);
        if (int rc = ensure_cub(r, tb)) return rc;
        RCHK(r, hipcub::DeviceSelect::Flagged(r->cub, tb, r->kept, r->flag, r->ring + r->P, r->nsel, (int)n, r->s));
        uint32_t nk = 0;
        RCHK(r, hipMemcpyAsync(&nk, r->nsel, 4, hipMemcpyDeviceToHost, r->s));
        RCHK(r, hipStreamSynchronize(r->s));
        const uint32_t P2 = r->P + nk;
        tb = 0;
        hipcub::DeviceRadixSort::SortKeys(nullptr, tb, r->ring, r->ring2, (int)P2, 0, 64, r->s);
        if (int rc = ensure_cub(r, tb)) return rc;
        RCHK(r, hipcub::DeviceRadixSort::SortKeys(r->cub, tb, r->ring, r->ring2, (int)P2, 0, 64, r->s));
        std::swap(r->ring, r->ring2);
        r->P = P2;
    }
    *adds_done = true;
    if (!D.empty() && r->P) {
        const uint32_t nd = (uint32_t)(D.size() * r->R);
        if (int rc = ensure_scratch(r, std::max<size_t>(r->P, nd))) return rc;   // before k1 is filled
        if (int rc = hash_replicas(r, D)) return rc;
        hipLaunchKernelGGL(k_ring_drop, dim3(grid_for(r->P)), dim3(256), 0, r->s, r->ring, r->P, r->k1, nd, r->flag);
        if (!r->nsel) RCHK(r, hipMalloc(&r->nsel, 16));
        size_t tb = 0;
        hipcub::DeviceSelect::Flagged(nullptr, tb, r->ring, r->flag, r->ring2, r->nsel, (int)r->P, r->s);
        if (int rc = ensure_cub(r, tb)) return rc;
        RCHK(r, hipcub::DeviceSelect::Flagged(r->cub, tb, r->ring, r->flag, r->ring2, r->nsel, (int)r->P, r->s));
        uint32_t nk = 0;
        RCHK(r, hipMemcpyAsync(&nk, r->nsel, 4, hipMemcpyDeviceToHost, r->s));
        RCHK(r, hipStreamSynchronize(r->s));
        std::swap(r->ring, r->ring2);
        r->P = nk;
    }
    RCHK(r, hipEventRecord(r->e1, r->s));
    RCHK(r, hipEventSynchronize(r->e1));
    float ms = 0;
    hipEventElapsedTime(&ms, r->e0, r->e1);
    r->t_add = ms;
    return 0;
}

int swimring_add_remove(swimring_t *r, const char *const *add, size_t nadd, const char *const *remove, size_t nremove,
                        int32_t *changed) {
    if (!r || (nadd && !add) || (nremove && !remove)) return SWIMSIM_EINVAL;
    if (changed) *changed = 0;
    // every name is checked and interned before the server set changes, so a bad name leaves the ring as
    // it was; a HIP failure further down rolls the set back to the servers the device ring holds
    for (size_t i = 0; i < nadd; i++)
        if (!add[i] || strlen(add[i]) > RING_NAME_MAX) return r->fail(SWIMSIM_EINVAL, "bad server name in the add list");
    for (size_t i = 0; i < nremove; i++)
        if (!remove[i]) return SWIMSIM_EINVAL;
    std::vector<int32_t> aid(nadd);
    for (size_t i = 0; i < nadd; i++)
        if (int rc = intern(r, add[i], &aid[i])) return rc;
    std::vector<int32_t> A, D;
    for (size_t i = 0; i < nadd; i++) {                          // addServerNoLock: skip servers in the set
        const int32_t id = aid[i];
        if (r->in_set[id]) continue;
        r->in_set[id] = 1;
        r->nset++;
        A.push_back(id);
    }
    for (size_t i = 0; i < nremove; i++) {                       // removeServerNoLock: skip unknown ones
        auto it = r->ids.find(remove[i]);
        if (it == r->ids.end() || !r->in_set[it->second]) continue;
        r->in_set[it->second] = 0;
        r->nset--;
        D.push_back(it->second);
    }
    if (A.empty() && D.empty()) return SWIMSIM_OK;
    if (changed) *changed = 1;
    auto undo = [&](bool adds, int rc) {
        if (adds)
            for (int32_t id : A) { r->in_set[id] = 0; r->nset--; }
        for (int32_t id : D) { r->in_set[id] = 1; r->nset++; }
        if (changed) *changed = 0;
        return rc;
    };
    if (int rc = sync_names(r)) return undo(true, rc);
    bool adds_done = false;
    if (int rc = ring_apply(r, A, D, &adds_done)) return undo(!adds_done, rc);
    return compute_checksum(r);
}

int swimring_checksum(swimring_t *r, uint32_t *out) {
    if (!r || !out) return SWIMSIM_EINVAL;
    *out = r->checksum;
    return SWIMSIM_OK;
}

int swimring_server_count(swimring_t *r, uint32_t *out) {
    if (!r || !out) return SWIMSIM_EINVAL;
    *out = r->nset;
    return SWIMSIM_OK;
}

int swimring_has_server(swimring_t *r, const char *server, int32_t *out) {
    if (!r || !server || !out) return SWIMSIM_EINVAL;
    auto it = r->ids.find(server);
    *out = it != r->ids.end() && r->in_set[it->second] ? 1 : 0;
    return SWIMSIM_OK;
}

int swimring_lookup_batch(swimring_t *r, const uint8_t *keys, const uint64_t *off, size_t nkeys, int32_t *out) {
    if (!r || !off || !out || (nkeys && !keys && off[nkeys])) return SWIMSIM_EINVAL;
    if (nkeys == 0) return SWIMSIM_OK;
    if (int rc = upload_keys(r, keys, off, nkeys)) return rc;
    RCHK(r, hipEventRecord(r->e0, r->s));
    hipLaunchKernelGGL(k_ring_lookup, dim3(grid_for(nkeys)), dim3(256), 0, r->s, r->bytes, r->boff, (uint32_t)nkeys,
                       r->ring, r->P, r->iout);
    RCHK(r, hipEventRecord(r->e1, r->s));
    RCHK(r, hipMemcpyAsync(out, r->iout, nkeys * 4, hipMemcpyDeviceToHost, r->s));
    RCHK(r, hipStreamSynchronize(r->s));
    float ms = 0;
    hipEventElapsedTime(&ms, r->e0, r->e1);
    r->t_look = ms;
    return SWIMSIM_OK;
}

int swimring_lookup_n(swimring_t *r, const uint8_t *key, size_t len, uint32_t n, int32_t *out, size_t *nout) {
    if (!r || (len && !key) || !out || !nout) return SWIMSIM_EINVAL;
    *nout = 0;
    if (n >= r->nset) {                                          // lookupNNoLock: every server
        for (size_t i = 0; i < r->names.size(); i++)
            if (r->in_set[i]) out[(*nout)++] = (int32_t)i;
        return SWIMSIM_OK;
    }
    if (n == 0) return SWIMSIM_OK;
    const uint64_t off[2] = {0, len};
    if (int rc = upload_keys(r, key, off, 1)) return rc;
    size_t c = r->out_cap, c2 = r->out_cap;
    if (int rc = grow(r, &r->iout, &c, n)) return rc;
    if (int rc = grow(r, &r->uout, &c2, n)) return rc;
    r->out_cap = std::min(c, c2);
    const size_t words = (r->names.size() + 31) / 32;
    if (words > r->seen_cap) {
        if (r->seen) hipFree(r->seen);
        r->seen = nullptr;
        r->seen_cap = 0;
        RCHK(r, hipMalloc(&r->seen, std::max<size_t>(words, 64) * 4));
        r->seen_cap = std::max<size_t>(words, 64);
    }
    hipLaunchKernelGGL(k_ring_lookup_n, dim3(1), dim3(256), 0, r->s, r->bytes, (uint32_t)len, r->ring, r->P, n, r->iout,
                       r->uout, r->seen, (uint32_t)words);
    uint32_t got = 0;
    RCHK(r, hipMemcpyAsync(&got, r->uout, 4, hipMemcpyDeviceToHost, r->s));
    RCHK(r, hipStreamSynchronize(r->s));
    RCHK(r, hipMemcpyAsync(out, r->iout, (size_t)got * 4, hipMemcpyDeviceToHost, r->s));
    RCHK(r, hipStreamSynchronize(r->s));
    *nout = got;
    return SWIMSIM_OK;
}

int swimring_lookup_n_batch(swimring_t *r, const uint8_t *keys, const uint64_t *off, size_t nkeys, uint32_t n,
                            int32_t *out, uint32_t *cnt) {
    if (!r || !off || !cnt) return SWIMSIM_EINVAL;
    if (nkeys == 0) return SWIMSIM_OK;
    if (!keys && off[nkeys]) return SWIMSIM_EINVAL;
    if (!replica_dims_ok(nkeys, n)) return r->fail(SWIMSIM_EINVAL, "nkeys * n exceeds 2^31 - 1 entries");
    if (n == 0) {
        memset(cnt, 0, nkeys * sizeof *cnt);
        return SWIMSIM_OK;
    }
    if (!out) return SWIMSIM_EINVAL;
    if (int rc = lookup_n_device(r, keys, off, nkeys, n)) return rc;
    RCHK(r, hipMemcpyAsync(out, r->mat, nkeys * n * 4, hipMemcpyDeviceToHost, r->s));
    RCHK(r, hipMemcpyAsync(cnt, r->uout, nkeys * 4, hipMemcpyDeviceToHost, r->s));
    RCHK(r, hipStreamSynchronize(r->s));
    return SWIMSIM_OK;
}

int swimring_group_replicas(swimring_t *r, const uint8_t *keys, const uint64_t *off, size_t nkeys, uint32_t n,
                            int32_t *out, uint32_t *cnt, int32_t *dest, uint64_t *dest_off, uint32_t *key_idx,
                            size_t *ndest) {
    if (!r || !off || !dest || !dest_off || !key_idx || !ndest) return SWIMSIM_EINVAL;
    *ndest = 0;
    dest_off[0] = 0;
    if (nkeys == 0) return SWIMSIM_OK;
    if (!keys && off[nkeys]) return SWIMSIM_EINVAL;
    if (!replica_dims_ok(nkeys, n)) return r->fail(SWIMSIM_EINVAL, "nkeys * n exceeds 2^31 - 1 entries");
    if (n == 0) {
        if (cnt) memset(cnt, 0, nkeys * sizeof *cnt);
        return SWIMSIM_OK;
    }
    if (int rc = lookup_n_device(r, keys, off, nkeys, n)) return rc;
    // sort (owner << 32 | key index) over the matrix, padding last; a destination starts where the owner changes
    const size_t total = nkeys * n;
    if (int rc = ensure_scratch(r, total)) return rc;
    if (!r->nsel) RCHK(r, hipMalloc(&r->nsel, 16));
    int idbits = 0;
    while (((size_t)1 << idbits) < r->names.size()) idbits++;     // ids < 2^idbits; one more bit orders the padding
    const int end_bit = std::min(64, 32 + idbits + 1);
    size_t tb = 0, tb2 = 0;
    hipcub::DeviceRadixSort::SortKeys(nullptr, tb, r->k0, r->k1, (int)total, 0, end_bit, r->s);
    hipcub::DeviceSelect::Flagged(nullptr, tb2, r->kept, r->flag, r->k0, r->nsel, (int)total, r->s);
    if (int rc = ensure_cub(r, std::max(tb, tb2))) return rc;
    RCHK(r, hipEventRecord(r->e0, r->s));
    hipLaunchKernelGGL(k_group_keys, dim3(grid_for(total)), dim3(256), 0, r->s, r->mat, n, (uint64_t)total, r->k0);
    RCHK(r, hipcub::DeviceRadixSort::SortKeys(r->cub, tb, r->k0, r->k1, (int)total, 0, end_bit, r->s));
    hipLaunchKernelGGL(k_group_bounds, dim3(grid_for(total)), dim3(256), 0, r->s, r->k1, (uint64_t)total, r->v0, r->flag,
                       r->kept);
    RCHK(r, hipcub::DeviceSelect::Flagged(r->cub, tb2, r->kept, r->flag, r->k0, r->nsel, (int)total, r->s));
    RCHK(r, hipEventRecord(r->e1, r->s));
    uint32_t nb = 0;
    RCHK(r, hipMemcpyAsync(&nb, r->nsel, 4, hipMemcpyDeviceToHost, r->s));
    RCHK(r, hipStreamSynchronize(r->s));
    float ms = 0;
    hipEventElapsedTime(&ms, r->e0, r->e1);
    r->t_group = ms;
    std::vector<unsigned long long> b(nb);
    if (nb) RCHK(r, hipMemcpyAsync(b.data(), r->k0, (size_t)nb * 8, hipMemcpyDeviceToHost, r->s));
    RCHK(r, hipStreamSynchronize(r->s));
    size_t nd = nb, valid = total;
    if (nb && (uint32_t)(b[nb - 1] >> 32) == 0xffffffffu) {       // the padding's run
        nd = nb - 1;
        valid = (uint32_t)b[nb - 1];
    }
    if (nd > r->nset) return r->fail(SWIMSIM_EHIP, "grouping found %zu destinations for %u servers", nd, r->nset);
    for (size_t d = 0; d < nd; d++) {
        dest[d] = (int32_t)(b[d] >> 32);
        dest_off[d] = (uint32_t)b[d];
    }
    dest_off[nd] = valid;
    *ndest = nd;
    if (valid) RCHK(r, hipMemcpyAsync(key_idx, r->v0, valid * 4, hipMemcpyDeviceToHost, r->s));
    if (out) RCHK(r, hipMemcpyAsync(out, r->mat, total * 4, hipMemcpyDeviceToHost, r->s));
    if (cnt) RCHK(r, hipMemcpyAsync(cnt, r->uout, nkeys * 4, hipMemcpyDeviceToHost, r->s));
    RCHK(r, hipStreamSynchronize(r->s));
    return SWIMSIM_OK;
}

int swimring_last_replica_times(swimring_t *r, double *lookup_n_ms, double *group_ms) {
    if (!r) return SWIMSIM_EINVAL;
    if (lookup_n_ms) *lookup_n_ms = r->t_lookn;
    if (group_ms) *group_ms = r->t_group;
    return SWIMSIM_OK;
}

const char *swimring_server_name(swimring_t *r, int32_t id) {
    if (!r || id < 0 || (size_t)id >= r->names.size()) return nullptr;
    return r->names[id].c_str();
}

int swimring_points(swimring_t *r, uint32_t *hash, int32_t *owner, size_t cap, size_t *n) {
    if (!r || !n) return SWIMSIM_EINVAL;
    *n = r->P;
    if (!hash && !owner) return SWIMSIM_OK;
    std::vector<unsigned long long> h(r->P);
    if (r->P) RCHK(r, hipMemcpyAsync(h.data(), r->ring, (size_t)r->P * 8, hipMemcpyDeviceToHost, r->s));
    RCHK(r, hipStreamSynchronize(r->s));
    for (size_t i = 0; i < h.size() && i < cap; i++) {
        if (hash) hash[i] = (uint32_t)(h[i] >> 32);
        if (owner) owner[i] = (int32_t)(uint32_t)h[i];
    }
    return SWIMSIM_OK;
}

int swimring_fingerprint32_batch(swimring_t *r, const uint8_t *bytes, const uint64_t *off, size_t n, uint32_t *out) {
    if (!r || !off || !out) return SWIMSIM_EINVAL;
    if (n == 0) return SWIMSIM_OK;
    if (int rc = upload_keys(r, bytes, off, n)) return rc;
    hipLaunchKernelGGL(k_fp32_batch, dim3(grid_for(n)), dim3(256), 0, r->s, r->bytes, r->boff, (uint32_t)n, r->uout);
    RCHK(r, hipMemcpyAsync(out, r->uout, n * 4, hipMemcpyDeviceToHost, r->s));
    RCHK(r, hipStreamSynchronize(r->s));
    return SWIMSIM_OK;
}

int swimring_last_times(swimring_t *r, double *add_remove_ms, double *lookup_ms) {
    if (!r) return SWIMSIM_EINVAL;
    if (add_remove_ms) *add_remove_ms = r->t_add;
    if (lookup_ms) *lookup_ms = r->t_look;
    return SWIMSIM_OK;
}

}  // extern "C"
