// The geometry digest's arithmetic, once, for the device (csrc/digest.hip: coords_digest_k, coords_digest_finish_k) and for the host
// (csrc/digest_host.cpp: linr_coords_digest_host): everything that decides a bit of a digest (include/linr_hip.h has the definition,
// linr_pcgc_amd/stream_digests.py the format).  Unsigned 64-bit integers that wrap, no floating point, so the sum over the rows is
// the same in any order: a grid of partial sums and a plain loop agree bit for bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DG_HD __host__ __device__ inline
#else
#define DG_HD inline
#endif

#define DG_GOLDEN 0x9E3779B97F4A7C15ull

// the splitmix64 finaliser: a bijection of the 64-bit words
DG_HD uint64_t dg_mix(uint64_t v) {
    v ^= v >> 30;
    v *= 0xBF58476D1CE4E5B9ull;
    v ^= v >> 27;
    v *= 0x94D049BB133111EBull;
    v ^= v >> 31;
    return v;
}

// one row's term; (x, y, z) = the row + the origin, added in int32 with wrap-around (through unsigned: no signed overflow)
DG_HD uint64_t dg_row(int32_t x, int32_t y, int32_t z, int32_t ox, int32_t oy, int32_t oz) {
    const uint32_t ux = (uint32_t)x + (uint32_t)ox, uy = (uint32_t)y + (uint32_t)oy, uz = (uint32_t)z + (uint32_t)oz;
    return dg_mix(dg_mix((uint64_t)ux | ((uint64_t)uy << 32)) + (uint64_t)uz + DG_GOLDEN);
}

// the digest of n rows whose terms sum to `sum`
DG_HD uint64_t dg_finish(uint64_t sum, uint64_t n) { return dg_mix(sum ^ dg_mix(n + DG_GOLDEN)); }
