// philox.h -- seed-addressed standard normals: Philox4x32-10 + Box-Muller, plain C++ for host and device.
//
// Philox4x32-10 as published (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of
//   (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),   the key bumped by the Weyl constants
// between rounds.  No state: the output is a function of (counter, key) alone.
//
// The noise contract of this library (DESIGN.md "Seed-addressed noise"; a compatibility contract):
//   key     = the request's 64-bit seed (lo32, hi32)
//   counter = (q, ordinal lo32, ordinal hi32, domain),  q = e / 4, e the element's flat NCHW index inside its image
//   the four output words r0..r3 give the elements 4q .. 4q+3:
//     u(r) = ((r >> 8) + 0.5f) * 2^-24          evaluated in fp32 (round to nearest even)
//     z[4q]   = sqrtf(-2 logf(u(r0))) cosf(2 pi u(r1)),  z[4q+1] = the same radius times sinf(...);  r2, r3 likewise for 4q+2, 4q+3
// u is exact for r >> 8 < 2^23; above, the sum has 25 significant bits and rounds to even, so u lies in (0, 1] and u = 1 (radius 0,
// a finite value) is reached by the single top value of r >> 8.  |z| <= sqrt(50 ln 2) = 5.89.
//
// Every kernel that needs noise calls philox_normal4 below and is compiled with -ffp-contract=off: a fused kernel and the fill
// kernel produce the same bits on the same device.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(HIPEMU)
#define BBDM_PHILOX_FN __host__ __device__ __forceinline__
#else
#define BBDM_PHILOX_FN inline
#endif

enum { BBDM_NOISE_P_SAMPLE = 0, BBDM_NOISE_Q_SAMPLE = 1 };     // the `domain` word of the counter

// (hi, lo) of the 32 x 32 -> 64 bit product: one v_mad_u64_u32 on gfx950 (both halves of the product are needed)
BBDM_PHILOX_FN void philox_mulhilo(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
    const uint64_t p = (uint64_t)a * (uint64_t)b;
    hi = (uint32_t)(p >> 32);
    lo = (uint32_t)p;
}

BBDM_PHILOX_FN void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t r[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        uint32_t hi0, lo0, hi1, lo1;
        philox_mulhilo(0xD2511F53u, c0, hi0, lo0);
        philox_mulhilo(0xCD9E8D57u, c2, hi1, lo1);
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = c0, r[1] = c1, r[2] = c2, r[3] = c3;
}

BBDM_PHILOX_FN float philox_u01(uint32_t r) { return ((float)(r >> 8) + 0.5f) * 0x1p-24f; }

BBDM_PHILOX_FN void philox_box_muller(uint32_t ra, uint32_t rb, float& z0, float& z1) {
    const float R = sqrtf(-2.0f * logf(philox_u01(ra)));
    const float th = 0x1.921fb6p+2f * philox_u01(rb);          // 2 pi
    z0 = R * cosf(th);
    z1 = R * sinf(th);
}

// The four normals of group q of one image: elements 4q .. 4q+3.  seed / ordinal: the image's int64 values as two's complement bits.
BBDM_PHILOX_FN void philox_normal4(int64_t seed, int64_t ordinal, uint32_t domain, uint32_t q, float z[4]) {
    uint32_t r[4];
    philox4x32_10(q, (uint32_t)(uint64_t)ordinal, (uint32_t)((uint64_t)ordinal >> 32), domain, (uint32_t)(uint64_t)seed,
                  (uint32_t)((uint64_t)seed >> 32), r);
    philox_box_muller(r[0], r[1], z[0], z[1]);
    philox_box_muller(r[2], r[3], z[2], z[3]);
}
