// What the HBM-bound elementwise files (bridge.hip, loss_meter.hip) share: the groups-of-four access, the grids of the flat and the
// one-image-per-blockIdx.y kernels, the fp64 workgroup sum and the loss term.  Every includer is built with -ffp-contract=off.
#pragma once
#include "common.h"

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

inline unsigned ew_blocks(size_t total) {
    size_t b = (total + 255) / 256;
    return (unsigned)(b > 8192 ? 8192 : (b ? b : 1));
}

// grid of the one-image-per-blockIdx.y kernels: groups of four elements, 256 per block
inline dim3 group_grid(int N, int per_sample) {
    const size_t b = ((size_t)per_sample + 1023) / 1024;
    return dim3((unsigned)(b > 2048 ? 2048 : b), (unsigned)N);
}

// A thread's group of four consecutive elements.  VEC: per_sample % 4 == 0 and 16-byte aligned pointers (the launchers check), one
// 128-bit access per tensor and group; otherwise element accesses with the image's tail (count < 4 elements) guarded.
template <bool VEC>
__device__ __forceinline__ void load_group(const float* __restrict__ p, int count, float v[4]) {
    if (VEC) {
        const float4 f = *reinterpret_cast<const float4*>(p);
        v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < count ? p[j] : 0.f;
    }
}

template <bool VEC>
__device__ __forceinline__ void store_group(float* __restrict__ p, int count, const float v[4]) {
    if (VEC) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < count) p[j] = v[j];
    }
}

// Sum over the 256 threads of a workgroup in a fixed order: a __shfl_down tree inside each wave, then (w0 + w1) + (w2 + w3).  The
// result is valid in thread 0.  A kernel that sums more than once puts a __syncthreads() between two calls (red is rewritten).
// NOT optim.hip's block_sum_fixed: that one is an xor butterfly, which adds in another order and rounds differently.
__device__ __forceinline__ double block_sum_down(double s) {
    __shared__ double red[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// One element's loss term (BrownianBridgeModel.py:114-117): the difference in fp32, |d| or d^2 widened to fp64 for the sum.
__device__ __forceinline__ double loss_term(float x, float y, int loss_type) {
    const float d = x - y;
    return loss_type == 0 ? (double)fabsf(d) : (double)d * (double)d;
}
