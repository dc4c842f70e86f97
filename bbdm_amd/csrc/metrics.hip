// metrics.hip -- evaluation metrics of a sample set, taken from the uint8 images on the device.
//
// The reference scores a checkpoint offline from the PNG files: evaluation/diversity.py:8-39 re-opens every file with PIL and forms the
// per-pixel standard deviation of the sample_num samples of a condition on the CPU; it has no paired metric at all.  The bytes of
// those files are what bbdm_images_to_u8_f32 (egress.hip) writes, NHWC, so the same numbers can be taken before anything leaves the
// device:
//   bbdm_u8_pair_sums   sum |a - b| and sum (a - b)^2 per image, exact 64-bit integers              (-> MAE, MSE, PSNR on the host)
//   bbdm_u8_ssim        the SSIM map of Wang et al. 2004 (11-tap window, valid positions), fp64, summed per image
//   bbdm_u8_diversity   sum over the elements of the fp32 standard deviation over the S samples, diversity.py:26-35 step by step
// Every result is a function of the input bytes alone: the integer sums are integer atomics; the fp64 / fp32 values of the other two are
// turned into FIXED-POINT integers per element (a fixed function of the value), summed as integers, and added into a stats_acc.h cell
// as exact limbs.  No floating-point sum crosses a thread, so no tile shape, grid size or arrival order can show in a bit.
// Built with -ffp-contract=off: the fp32 sequence of the diversity is the reference's operation by operation; every fused step of the
// SSIM moments is written as fma().
#include "common.h"
#include "stats_acc.h"

namespace {

typedef unsigned long long u64;

// sum of `v` over the 256 threads of the block (integers: any order gives the same bits); valid in thread 0
__device__ __forceinline__ long long block_sum_256(long long v, long long* red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// cell += q * 2^-frac, exactly, for 0 <= |q| < 2^62 and 40 <= frac <= 52: the two halves of q are doubles without rounding and
// multiples of the cell's resolution 2^-70, so sa_add's decomposition drops nothing
__device__ __forceinline__ void sa_add_fixed(u64* cell, long long q, double unit_hi, double unit_lo) {
    const long long hi = q >> 30, lo = q & 0x3fffffffll;          // q = hi * 2^30 + lo, 0 <= lo < 2^30 (arithmetic shift: also q < 0)
    sa_add(cell, (double)hi * unit_hi);
    sa_add(cell, (double)lo * unit_lo);
}

// ---- pair sums ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void acc_word(unsigned wa, unsigned wb, unsigned& s1, unsigned& s2) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = (int)((wa >> (8 * k)) & 255u) - (int)((wb >> (8 * k)) & 255u);
        s1 += (unsigned)(d < 0 ? -d : d);
        s2 += (unsigned)(d * d);
    }
}

constexpr int PS_CHUNK = 16384;          // bytes of one image per workgroup: 64 per thread, 4 x 16-byte loads

// grid (chunks of the image, N).  The two images of a pair are read as 16-byte words where both pointers are congruent mod 16, as
// 4-byte words where they are congruent mod 4, else byte by byte; the bytes in front of the first aligned word and behind the last
// whole word are the element head / tail (chunk 0 takes them).  Per-thread sums are 32-bit: at most 64 + 1 bytes x 65025.
__global__ void __launch_bounds__(256) u8_pair_sums_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b,
                                                           u64* __restrict__ out, size_t L) {
    __shared__ long long red[2][4];
    const int n = blockIdx.y, tid = threadIdx.x;
    const unsigned char* pa = a + (size_t)n * L;
    const unsigned char* pb = b + (size_t)n * L;
    const uintptr_t ua = (uintptr_t)pa, ub = (uintptr_t)pb;
    const int wbytes = ((ua ^ ub) & 15) == 0 ? 16 : ((ua ^ ub) & 3) == 0 ? 4 : 1;
    size_t head = (size_t)((wbytes - (ua & (wbytes - 1))) & (wbytes - 1));
    if (head > L) head = L;
    const size_t nwords = (L - head) / wbytes, tail0 = head + nwords * wbytes;
    long long t1 = 0, t2 = 0;
    if (blockIdx.x == 0) {                                       // head and tail: fewer than 2 x 16 bytes
        unsigned s1 = 0, s2 = 0;
        for (size_t i = tid; i < head + (L - tail0); i += 256) {
            const size_t e = i < head ? i : tail0 + (i - head);
            const int d = (int)pa[e] - (int)pb[e];
            s1 += (unsigned)(d < 0 ? -d : d);
            s2 += (unsigned)(d * d);
        }
        t1 += s1;
        t2 += s2;
    }
    const size_t wpc = PS_CHUNK / wbytes;                        // words per chunk
    const size_t w0 = blockIdx.x * wpc;
    if (w0 < nwords) {
        const size_t w1 = w0 + wpc < nwords ? w0 + wpc : nwords;
        unsigned s1 = 0, s2 = 0;
        if (wbytes == 16) {
            const uint4* qa = reinterpret_cast<const uint4*>(pa + head);
            const uint4* qb = reinterpret_cast<const uint4*>(pb + head);
            for (size_t w = w0 + tid; w < w1; w += 256) {
                const uint4 x = qa[w], y = qb[w];
                acc_word(x.x, y.x, s1, s2);
                acc_word(x.y, y.y, s1, s2);
                acc_word(x.z, y.z, s1, s2);
                acc_word(x.w, y.w, s1, s2);
            }
        } else if (wbytes == 4) {
            const unsigned* qa = reinterpret_cast<const unsigned*>(pa + head);
            const unsigned* qb = reinterpret_cast<const unsigned*>(pb + head);
            for (size_t w = w0 + tid; w < w1; w += 256) acc_word(qa[w], qb[w], s1, s2);
        } else {
            for (size_t w = w0 + tid; w < w1; w += 256) {
                const int d = (int)pa[head + w] - (int)pb[head + w];
                s1 += (unsigned)(d < 0 ? -d : d);
                s2 += (unsigned)(d * d);
            }
        }
        t1 += s1;
        t2 += s2;
    }
    const long long b1 = block_sum_256(t1, red[0]);
    const long long b2 = block_sum_256(t2, red[1]);
    if (tid == 0) {
        if (b1) atomicAdd(out + (size_t)n * 2, (u64)b1);
        if (b2) atomicAdd(out + (size_t)n * 2 + 1, (u64)b2);
    }
}

// ---- SSIM --------------------------------------------------------------------------------------------------------------------
constexpr int SS_WIN = 11;
constexpr int SS_TH = 16, SS_TW = 32;                            // window positions (output rows x columns) per workgroup
constexpr int SS_IH = SS_TH + SS_WIN - 1, SS_IW = SS_TW + SS_WIN - 1;
constexpr int SS_IWP = SS_IW + 2;                                // row pitch of the staged bytes
struct SsimWindow {
    double v[SS_WIN];
};

// grid (column tiles x row tiles, C, N), 256 threads.  One channel of the tile + its 10-pixel halo is staged as bytes; the horizontal
// pass forms the five window moments (x, y, x^2, y^2, x y: the products are integers, exact in fp64) of every staged row at every output
// column, one thread per (row, column) with the taps in the order 0..10; the vertical pass does the same down the columns and evaluates
// the map.  The value at a window position is therefore the same expression of the same 2 x 121 bytes wherever the position falls in a
// tile.  It is cut to a multiple of 2^-52 (|map| <= 1: at most one fp64 rounding unit) and summed as a 64-bit integer.
__global__ void __launch_bounds__(256) u8_ssim_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b,
                                                      u64* __restrict__ cells, int H, int W, int C, int tiles_x, SsimWindow win) {
    __shared__ unsigned char xs[SS_IH][SS_IWP], ys[SS_IH][SS_IWP];
    __shared__ double hm[5][SS_IH][SS_TW];
    __shared__ long long red[4];
    const int tid = threadIdx.x, ch = blockIdx.y, n = blockIdx.z;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int r0 = ty * SS_TH, c0 = tx * SS_TW;
    const size_t img = (size_t)n * H * W * C;
    for (int i = tid; i < SS_IH * SS_IW; i += 256) {
        const int r = i / SS_IW, c = i - r * SS_IW;
        const int y = r0 + r, x = c0 + c;
        unsigned char va = 0, vb = 0;                            // outside the image: feeds only window positions that are masked below
        if (y < H && x < W) {
            const size_t e = img + ((size_t)y * W + x) * C + ch;
            va = a[e];
            vb = b[e];
        }
        xs[r][c] = va;
        ys[r][c] = vb;
    }
    __syncthreads();
    for (int i = tid; i < SS_IH * SS_TW; i += 256) {
        const int r = i / SS_TW, c = i - r * SS_TW;
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
        for (int j = 0; j < SS_WIN; ++j) {
            const int x = xs[r][c + j], y = ys[r][c + j];
            const double w = win.v[j];
            m0 = fma(w, (double)x, m0);
            m1 = fma(w, (double)y, m1);
            m2 = fma(w, (double)(x * x), m2);
            m3 = fma(w, (double)(y * y), m3);
            m4 = fma(w, (double)(x * y), m4);
        }
        hm[0][r][c] = m0;
        hm[1][r][c] = m1;
        hm[2][r][c] = m2;
        hm[3][r][c] = m3;
        hm[4][r][c] = m4;
    }
    __syncthreads();
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    long long q = 0;
    for (int i = tid; i < SS_TH * SS_TW; i += 256) {
        const int r = i / SS_TW, c = i - r * SS_TW;
        if (r0 + r >= H - (SS_WIN - 1) || c0 + c >= W - (SS_WIN - 1)) continue;
        double mx = 0.0, my = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
#pragma unroll
        for (int j = 0; j < SS_WIN; ++j) {
            const double w = win.v[j];
            mx = fma(w, hm[0][r + j][c], mx);
            my = fma(w, hm[1][r + j][c], my);
            exx = fma(w, hm[2][r + j][c], exx);
            eyy = fma(w, hm[3][r + j][c], eyy);
            exy = fma(w, hm[4][r + j][c], exy);
        }
        const double mxx = mx * mx, myy = my * my, mxy = mx * my;
        const double sxx = exx - mxx, syy = eyy - myy, sxy = exy - mxy;
        const double num = (2.0 * mxy + C1) * (2.0 * sxy + C2);
        const double den = (mxx + myy + C1) * (sxx + syy + C2);
        const double map = num / den;
        // |map| <= 1 up to rounding; a wider value (NaN: a non-finite window) is kept out of the integer and marks the cell instead
        if (fabs(map) <= 2.0) q += (long long)(map * 0x1p52);
        else atomicAdd(cells + (size_t)n * SA_W + 3, 1ull);
    }
    const long long bq = block_sum_256(q, red);                  // at most 512 values of 2^52 (1 + 2^-52): below 2^62
    if (tid == 0) sa_add_fixed(cells + (size_t)n * SA_W, bq, 0x1p-22, 0x1p-52);
}

__global__ void u8_cells_read_kernel(const u64* __restrict__ cells, double* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = sa_load(cells + (size_t)i * SA_W);
}

// ---- diversity ---------------------------------------------------------------------------------------------------------------
// grid (cdiv(E / V, 256), M): one thread = V consecutive elements of one condition (V = 4: one 32-bit load per sample), its S samples
// read twice (mean, then variance: the second pass hits the cache).  The fp32 sequence is evaluation/diversity.py:26-35 (header); with
// S <= 65536 the sum of the bytes stays below 2^24 and is exact, so equal samples give mean = v and a standard deviation of exactly 0.
// Samples that are not all equal: their squared deviations from ANY centre sum to at least those from the exact mean, (S - 1) / S
// >= 1/2, so the standard deviation is at least about sqrt(1 / (2 S)) >= 2^-9 (and at most 127.5): an fp32 value there is a multiple
// of 2^-33, std * 2^40 is an integer below 2^47 without rounding, and the 1024 of a workgroup fit a 64-bit sum.
template <int V>
__global__ void __launch_bounds__(256) u8_diversity_kernel(const unsigned char* __restrict__ x, u64* __restrict__ cells, int S, size_t E) {
    __shared__ long long red[4];
    const int m = blockIdx.y;
    const size_t e0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * V;
    const unsigned char* px = x + (size_t)m * S * E + e0;
    long long q = 0;
    if (e0 < E) {
        const float fs = (float)S;
        float mean[V], var[V];
#pragma unroll
        for (int k = 0; k < V; ++k) mean[k] = 0.f, var[k] = 0.f;
        for (int j = 0; j < S; ++j) {
            unsigned w;
            if (V == 4) w = *reinterpret_cast<const unsigned*>(px + (size_t)j * E);
            else w = px[(size_t)j * E];
#pragma unroll
            for (int k = 0; k < V; ++k) mean[k] = mean[k] + (float)((w >> (8 * k)) & 255u);
        }
#pragma unroll
        for (int k = 0; k < V; ++k) mean[k] = mean[k] / fs;
        for (int j = 0; j < S; ++j) {
            unsigned w;
            if (V == 4) w = *reinterpret_cast<const unsigned*>(px + (size_t)j * E);
            else w = px[(size_t)j * E];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float d = (float)((w >> (8 * k)) & 255u) - mean[k];
                var[k] = var[k] + d * d;
            }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float sd = sqrtf(var[k] / fs);
            q += (long long)((double)sd * 0x1p40);
        }
    }
    const long long bq = block_sum_256(q, red);
    if (threadIdx.x == 0) sa_add_fixed(cells + (size_t)m * SA_W, bq, 0x1p-10, 0x1p-40);
}

int cells_read(const void* cells, double* out, int n, void* stream, const char* what) {
    BBDM_REQUIRE(cells && out && n > 0, "%s: bad args", what);
    hipLaunchKernelGGL(u8_cells_read_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (const u64*)cells, out, n);
    BBDM_CHECK_LAUNCH(what);
    return BBDM_OK;
}

}  // namespace

extern "C" int bbdm_u8_pair_sums(const unsigned char* a, const unsigned char* b, unsigned long long* out, int N, int H, int W, int C,
                                 void* stream) {
    BBDM_REQUIRE(a && b && out && N > 0 && H > 0 && W > 0 && C > 0, "u8_pair_sums: bad args");
    BBDM_REQUIRE(N <= 65535, "u8_pair_sums: N=%d > 65535", N);
    const size_t L = (size_t)H * W * C;
    const size_t chunks = (L + PS_CHUNK - 1) / PS_CHUNK;
    BBDM_REQUIRE(chunks < ((size_t)1 << 31), "u8_pair_sums: H x W x C too large");
    hipLaunchKernelGGL(u8_pair_sums_kernel, dim3((unsigned)chunks, N), dim3(256), 0, (hipStream_t)stream, a, b, out, L);
    BBDM_CHECK_LAUNCH("u8_pair_sums");
    return BBDM_OK;
}

extern "C" int bbdm_u8_ssim(const unsigned char* a, const unsigned char* b, const double* w, unsigned long long* cells, int N, int H,
                            int W, int C, void* stream) {
    BBDM_REQUIRE(a && b && w && cells && N > 0 && C > 0, "u8_ssim: bad args");
    BBDM_REQUIRE(H >= SS_WIN && W >= SS_WIN, "u8_ssim: H=%d W=%d, the window needs at least %d x %d", H, W, SS_WIN, SS_WIN);
    BBDM_REQUIRE(N <= 65535 && C <= 65535, "u8_ssim: N=%d C=%d > 65535", N, C);
    BBDM_REQUIRE((long long)H * W < (1ll << 31), "u8_ssim: H x W too large");
    SsimWindow win;
    for (int j = 0; j < SS_WIN; ++j) win.v[j] = w[j];
    const int tiles_x = cdiv(W - (SS_WIN - 1), SS_TW), tiles_y = cdiv(H - (SS_WIN - 1), SS_TH);
    hipLaunchKernelGGL(u8_ssim_kernel, dim3((unsigned)(tiles_x * tiles_y), C, N), dim3(256), 0, (hipStream_t)stream, a, b, cells, H, W, C,
                       tiles_x, win);
    BBDM_CHECK_LAUNCH("u8_ssim");
    return BBDM_OK;
}

extern "C" int bbdm_u8_ssim_read(const unsigned long long* cells, double* out, int N, void* stream) {
    return cells_read(cells, out, N, stream, "u8_ssim_read");
}

extern "C" int bbdm_u8_diversity(const unsigned char* x, unsigned long long* cells, int M, int S, int H, int W, int C, void* stream) {
    BBDM_REQUIRE(x && cells && M > 0 && S > 0 && H > 0 && W > 0 && C > 0, "u8_diversity: bad args");
    BBDM_REQUIRE(M <= 65535 && S <= (1 << 16), "u8_diversity: M=%d > 65535 or S=%d > 65536", M, S);
    const size_t E = (size_t)H * W * C;
    BBDM_REQUIRE(E < ((size_t)1 << 33), "u8_diversity: H x W x C too large");
    if (E % 4 == 0 && ((uintptr_t)x & 3) == 0)
        hipLaunchKernelGGL(u8_diversity_kernel<4>, dim3((unsigned)((E / 4 + 255) / 256), M), dim3(256), 0, (hipStream_t)stream, x, cells, S,
                           E);
    else
        hipLaunchKernelGGL(u8_diversity_kernel<1>, dim3((unsigned)((E + 255) / 256), M), dim3(256), 0, (hipStream_t)stream, x, cells, S, E);
    BBDM_CHECK_LAUNCH("u8_diversity");
    return BBDM_OK;
}

extern "C" int bbdm_u8_diversity_read(const unsigned long long* cells, double* out, int M, void* stream) {
    return cells_read(cells, out, M, stream, "u8_diversity_read");
}
