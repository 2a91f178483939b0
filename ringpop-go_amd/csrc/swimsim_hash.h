// swimsim_hash.h — go-farm Fingerprint32 of one string per lane and the ring's replica strings, shared by the ring
// (swimring.hip) and the engine's route kernels (swimsim_route.hip).
#pragma once
#include "swimsim_device.h"

namespace swimdev {

// ---------------------------------------------------------------------------------------------
// go-farm Fingerprint32 (FarmHash-32 "mk", glide.lock:18-19), one string per lane. Bytes come from
// a per-lane buffer, so the length paths select only arithmetic.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ld32(const uint8_t *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ __forceinline__ uint32_t fmix_fh(uint32_t h) {
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

__device__ inline uint32_t fp32_dev(const uint8_t *s, uint32_t len) {
    if (len <= 4) {                                               // Hash32Len0to4
        uint32_t b = 0, c = 9;
        for (uint32_t i = 0; i < len; i++) {
            b = b * FH_C1 + (uint32_t)(int32_t)(int8_t)s[i];
            c ^= b;
        }
        return fmix_fh(fh_mur(b, fh_mur(len, c)));
    }
    if (len <= 12) {                                              // Hash32Len5to12
        uint32_t a = len, b = len * 5, c = 9, d = b;
        a += ld32(s);
        b += ld32(s + len - 4);
        c += ld32(s + ((len >> 1) & 4));
        return fmix_fh(fh_mur(c, fh_mur(b, fh_mur(a, d))));
    }
    if (len <= 24) {                                              // Hash32Len13to24
        uint32_t a = ld32(s - 4 + (len >> 1)), b = ld32(s + 4), c = ld32(s + len - 8);
        uint32_t d = ld32(s + (len >> 1)), e = ld32(s), f = ld32(s + len - 4);
        uint32_t h = d * FH_C1 + len;
        a = ror32(a, 12) + f;
        h = fh_mur(c, h) + a;
        a = ror32(a, 3) + c;
        h = fh_mur(e, h) + a;
        a = ror32(a + f, 12) + d;
        h = fh_mur(b, h) + a;
        return fmix_fh(h);
    }
    FH fh;                                                        // len > 24: prologue, 20-byte blocks
    fh.init(len, ld32(s + len - 20), ld32(s + len - 16), ld32(s + len - 12), ld32(s + len - 8), ld32(s + len - 4));
    const uint32_t iters = (len - 1) / 20;
    for (uint32_t k = 0; k < iters; k++, s += 20)
        fh.block(ld32(s), ld32(s + 4), ld32(s + 8), ld32(s + 12), ld32(s + 16));
    return fh.fin();
}

// name ‖ decimal(i) into buf; returns its length (fmt.Sprintf("%s%v", server, i), hashring.go:151)
__device__ __forceinline__ uint32_t replica_string(const uint8_t *name, uint32_t nlen, uint32_t i, uint8_t *buf) {
    for (uint32_t k = 0; k < nlen; k++) buf[k] = name[k];
    uint8_t dig[10];
    uint32_t nd = 0;
    do { dig[nd++] = (uint8_t)('0' + i % 10u); i /= 10u; } while (i);
    for (uint32_t k = 0; k < nd; k++) buf[nlen + k] = dig[nd - 1 - k];
    return nlen + nd;
}

__device__ __forceinline__ uint32_t lower_bound_u64(const unsigned long long *a, uint32_t n, unsigned long long x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

}  // namespace swimdev
