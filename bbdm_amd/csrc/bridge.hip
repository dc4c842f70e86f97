// bridge.hip -- Brownian-Bridge scheduler arithmetic and tensor-layout glue (HBM-bound elementwise kernels).
//
// Replaces q_sample (BBM.py:128-146), predict_x0_from_objective (:148-160), the p_sample update (:186-201), the
// L1/L2 loss reduction (:114-117), extract() (model/utils.py:4-7, folded in: kernels read the schedule tables
// directly), th.cat([x, context], 1) (openaimodel.py:742) and the NCHW<->NHWC hand-over at the UNet boundary.
// Compiled with -ffp-contract=off: the reference evaluates these formulas as separate fp32 tensor ops.
#include "common.h"
#include "dispatch.h"
#include "elementwise.h"
#include "philox.h"
#include "stats_acc.h"

namespace {

__device__ __forceinline__ float predict_x0_one(int objective, float x_t, float y, float pred, float m, float sig) {
    if (objective == 0) return x_t - pred;
    if (objective == 1) return (x_t - m * y - sig * pred) / (1.f - m);
    return y - pred;
}

// q_sample of one element (BBM.py:128-146): x_t and the target of the objective.
struct QSample {
    float x_t, target;
};

__device__ __forceinline__ QSample q_sample_one(int objective, float m, float sig, float a, float b, float e) {
    QSample r;
    if (objective == 0) r.target = m * (b - a) + sig * e;
    else if (objective == 1) r.target = e;
    else r.target = b - a;
    r.x_t = (1.f - m) * a + m * b + sig * e;
    return r;
}

// The coefficients of one bridge step t -> t_next (BBM.py:186-201); a last step uses m_t and sig_obj alone and ignores t_next and eta.
struct StepCoef {
    float m_t, sig_obj, m_nt, sigma_t, coef;
};

__device__ __forceinline__ StepCoef step_coef(const float* __restrict__ m_tab, const float* __restrict__ var_tab, int64_t t,
                                              int64_t t_next, int is_last, float eta) {
    StepCoef c;
    c.m_t = m_tab[t];
    const float var_t = var_tab[t];
    c.sig_obj = sqrtf(var_t);
    c.m_nt = 0.f, c.sigma_t = 0.f, c.coef = 0.f;
    if (!is_last) {
        c.m_nt = m_tab[t_next];
        const float var_nt = var_tab[t_next];
        // sigma2_t = (var_t - var_nt * (1 - m_t)**2 / (1 - m_nt)**2) * var_nt / var_t       (BBM.py:194)
        const float a = (1.f - c.m_t) * (1.f - c.m_t);
        const float b = (1.f - c.m_nt) * (1.f - c.m_nt);
        const float sigma2 = (var_t - var_nt * a / b) * var_nt / var_t;
        c.sigma_t = sqrtf(sigma2) * eta;
        c.coef = sqrtf((var_nt - sigma2) / var_t);
    }
    return c;
}

// The step of one element: x0 by objective, clip, then the last step's x_next = x0_recon or the mean + sigma_t * noise.
struct StepOut {
    float x0_recon, x_next;
};

__device__ __forceinline__ StepOut step_one(const StepCoef& c, int objective, int clip, int is_last, float xt, float yy, float pred,
                                            float noise) {
    StepOut r;
    r.x0_recon = predict_x0_one(objective, xt, yy, pred, c.m_t, c.sig_obj);
    if (clip) r.x0_recon = fminf(fmaxf(r.x0_recon, -1.f), 1.f);
    if (is_last) {
        r.x_next = r.x0_recon;
    } else {
        // (1 - m_nt) x0 + m_nt y + sqrt((var_nt - sigma2)/var_t) (x_t - (1 - m_t) x0 - m_t y) + sigma_t eps
        const float mean = (1.f - c.m_nt) * r.x0_recon + c.m_nt * yy + c.coef * (xt - (1.f - c.m_t) * r.x0_recon - c.m_t * yy);
        r.x_next = mean + c.sigma_t * noise;
    }
    return r;
}

__global__ void q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ y,
                                const float* __restrict__ noise, const int64_t* __restrict__ t,
                                const float* __restrict__ m_t, const float* __restrict__ var_t,
                                float* __restrict__ x_t, float* __restrict__ target, int per_sample, size_t total,
                                int objective) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int n = (int)(i / per_sample);
        const int64_t tt = t[n];
        const float m = m_t[tt];
        const float sig = sqrtf(var_t[tt]);
        const QSample r = q_sample_one(objective, m, sig, x0[i], y[i], noise[i]);
        x_t[i] = r.x_t;
        target[i] = r.target;
    }
}

__global__ void predict_x0_kernel(const float* __restrict__ x_t, const float* __restrict__ y,
                                  const float* __restrict__ pred, const int64_t* __restrict__ t,
                                  const float* __restrict__ m_t, const float* __restrict__ var_t,
                                  float* __restrict__ x0r, int per_sample, size_t total, int objective) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int n = (int)(i / per_sample);
        const int64_t tt = t[n];
        x0r[i] = predict_x0_one(objective, x_t[i], y[i], pred[i], m_t[tt], sqrtf(var_t[tt]));
    }
}

__global__ void p_step_kernel(const float* __restrict__ x_t, const float* __restrict__ y, const float* __restrict__ pred,
                              const float* __restrict__ noise, const float* __restrict__ m_tab,
                              const float* __restrict__ var_tab, int t, int t_next, int is_last, float eta, int clip,
                              int objective, float* __restrict__ x_next, float* __restrict__ x0_recon,
                              float* __restrict__ x_next_alias, size_t total) {
    const StepCoef c = step_coef(m_tab, var_tab, t, t_next, is_last, eta);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const StepOut r = step_one(c, objective, clip, is_last, x_t[i], y[i], pred[i], is_last ? 0.f : noise[i]);   // no noise read by a last step
        x0_recon[i] = r.x0_recon;
        x_next[i] = r.x_next;
        if (x_next_alias) x_next_alias[i] = r.x_next;      // second copy: the caller's input buffer of the NEXT step (see the header)
    }
}

// Where a per-image launch takes eta and the clip decision of image n from -- the P of the two kernels below.
// UniformParams: one launch argument each, and the flag word is the state (the kernel arguments of the *_batched_ / *_philox_ entry
// points, unchanged).  RequestParams (the *_requests_* entry points): eta[n] from a device array (every active image reads its
// entry and its next step; a last step ignores both); bits 0-1 of the flag word are the state and bit 2 says "clip this image".
struct UniformParams {
    float eta_;
    int clip_;
    __device__ __forceinline__ int64_t state(int64_t flag) const { return flag; }
    __device__ __forceinline__ float eta(int) const { return eta_; }
    __device__ __forceinline__ int clip(int64_t) const { return clip_; }
};

struct RequestParams {
    const float* eta_;
    __device__ __forceinline__ int64_t state(int64_t flag) const { return flag & 3; }
    __device__ __forceinline__ float eta(int n) const { return eta_[n]; }
    __device__ __forceinline__ int clip(int64_t flag) const { return (int)(flag >> 2) & 1; }
};

// p_step_kernel with a (step, next step, flag) per image: one image per blockIdx.y, so the coefficients are evaluated once
// per thread and image.  State 0: a step with noise, 1: the last step (x_next = x0_recon, no noise read), 2: an inactive slot
// (nothing read or written).  The float expressions are p_step_kernel's, in the same order: an image whose (t, t_next, last, eta,
// clip) equals a scalar launch's gets the scalar kernel's bits.
template <class P>
__global__ void p_step_batched_kernel(const float* __restrict__ x_t, const float* __restrict__ y,
                                      const float* __restrict__ pred, const float* __restrict__ noise,
                                      const float* __restrict__ m_tab, const float* __restrict__ var_tab,
                                      const int64_t* __restrict__ t_arr, const int64_t* __restrict__ t_next_arr,
                                      const int64_t* __restrict__ flag_arr, P params, int objective,
                                      float* __restrict__ x_next, float* __restrict__ x0_recon,
                                      float* __restrict__ x_next_alias, int per_sample) {
    const int n = blockIdx.y;
    const int64_t flag = flag_arr[n];
    const int64_t state = params.state(flag);
    if (state == 2) return;
    const int is_last = state == 1;
    const int clip = params.clip(flag);
    const StepCoef c = step_coef(m_tab, var_tab, t_arr[n], t_next_arr[n], is_last, params.eta(n));
    const size_t base = (size_t)n * per_sample;
    for (size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x; k < (size_t)per_sample; k += (size_t)gridDim.x * blockDim.x) {
        const size_t i = base + k;
        const StepOut r = step_one(c, objective, clip, is_last, x_t[i], y[i], pred[i], is_last ? 0.f : noise[i]);
        x0_recon[i] = r.x0_recon;
        x_next[i] = r.x_next;
        if (x_next_alias) x_next_alias[i] = r.x_next;
    }
}

// ---- seed-addressed noise (philox.h): the normals are a function of (seed, ordinal, domain, element) and never touch memory in the
// fused kernels.  One image per blockIdx.y; a thread owns groups of four consecutive elements of it (one Philox call per group:
// its four words are the group's four normals).  VEC: per_sample % 4 == 0 and 16-byte aligned pointers (the launchers check), one
// 128-bit access per tensor and group; otherwise element accesses with the image's tail (per_sample % 4 elements) guarded
// (load_group / store_group of elementwise.h).
template <bool VEC>
__global__ void __launch_bounds__(256) philox_normal_kernel(float* __restrict__ out, const int64_t* __restrict__ seed_arr,
                                                            const int64_t* __restrict__ ordinal_arr, unsigned domain,
                                                            int per_sample) {
    const int n = blockIdx.y;
    const int64_t seed = seed_arr[n], ordinal = ordinal_arr[n];
    float* o = out + (size_t)n * per_sample;
    const unsigned groups = ((unsigned)per_sample + 3u) / 4u;
    for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < groups; q += gridDim.x * 256u) {
        float z[4];
        philox_normal4(seed, ordinal, domain, q, z);
        store_group<VEC>(o + 4 * (size_t)q, per_sample - (int)(4u * q), z);
    }
}

// Debug / test entry: the raw Philox4x32-10 words of n (counter, key) pairs through the device build of philox.h.
__global__ void philox_raw_kernel(const uint32_t* __restrict__ ck, uint32_t* __restrict__ out, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        uint32_t r[4];
        philox4x32_10(ck[6 * i], ck[6 * i + 1], ck[6 * i + 2], ck[6 * i + 3], ck[6 * i + 4], ck[6 * i + 5], r);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[4 * i + j] = r[j];
    }
}

// p_step_batched_kernel with the noise generated in registers (domain 0): the same (t, t_next, flag) per image and the same float
// expressions in the same order, so it equals p_step_batched_kernel fed philox_normal_kernel's tensor bit for bit.  Last-step and
// inactive images generate nothing.
template <bool VEC, class P>
__global__ void __launch_bounds__(256) p_step_philox_kernel(const float* __restrict__ x_t, const float* __restrict__ y,
                                                            const float* __restrict__ pred, const int64_t* __restrict__ seed_arr,
                                                            const int64_t* __restrict__ ordinal_arr,
                                                            const float* __restrict__ m_tab, const float* __restrict__ var_tab,
                                                            const int64_t* __restrict__ t_arr,
                                                            const int64_t* __restrict__ t_next_arr,
                                                            const int64_t* __restrict__ flag_arr, P params,
                                                            int objective, float* __restrict__ x_next,
                                                            float* __restrict__ x0_recon, float* __restrict__ x_next_alias,
                                                            int per_sample) {
    const int n = blockIdx.y;
    const int64_t flag = flag_arr[n];
    const int64_t state = params.state(flag);
    if (state == 2) return;
    const int is_last = state == 1;
    const int clip = params.clip(flag);
    const int64_t seed = seed_arr[n], ordinal = ordinal_arr[n];      // (a last step reads them too, and generates nothing)
    const StepCoef c = step_coef(m_tab, var_tab, t_arr[n], t_next_arr[n], is_last, params.eta(n));
    const size_t base = (size_t)n * per_sample;
    const unsigned groups = ((unsigned)per_sample + 3u) / 4u;
    for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < groups; q += gridDim.x * 256u) {
        const size_t i = base + 4 * (size_t)q;
        const int count = per_sample - (int)(4u * q);          // >= 4 except in the image's last group
        float xt[4], yy[4], pr[4], z[4] = {0.f, 0.f, 0.f, 0.f}, x0v[4], xnv[4];
        load_group<VEC>(x_t + i, count, xt);
        load_group<VEC>(y + i, count, yy);
        load_group<VEC>(pred + i, count, pr);
        if (!is_last) philox_normal4(seed, ordinal, BBDM_NOISE_P_SAMPLE, q, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const StepOut r = step_one(c, objective, clip, is_last, xt[j], yy[j], pr[j], z[j]);
            x0v[j] = r.x0_recon;
            xnv[j] = r.x_next;
        }
        store_group<VEC>(x0_recon + i, count, x0v);
        store_group<VEC>(x_next + i, count, xnv);
        if (x_next_alias) store_group<VEC>(x_next_alias + i, count, xnv);
    }
}

// q_sample_kernel with the noise generated in registers (domain 1), one image per blockIdx.y.
template <bool VEC>
__global__ void __launch_bounds__(256) q_sample_philox_kernel(const float* __restrict__ x0, const float* __restrict__ y,
                                                              const int64_t* __restrict__ seed_arr,
                                                              const int64_t* __restrict__ ordinal_arr,
                                                              const int64_t* __restrict__ t, const float* __restrict__ m_t,
                                                              const float* __restrict__ var_t, float* __restrict__ x_t,
                                                              float* __restrict__ target, int per_sample, int objective) {
    const int n = blockIdx.y;
    const int64_t tt = t[n];
    const float m = m_t[tt];
    const float sig = sqrtf(var_t[tt]);
    const int64_t seed = seed_arr[n], ordinal = ordinal_arr[n];
    const size_t base = (size_t)n * per_sample;
    const unsigned groups = ((unsigned)per_sample + 3u) / 4u;
    for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < groups; q += gridDim.x * 256u) {
        const size_t i = base + 4 * (size_t)q;
        const int count = per_sample - (int)(4u * q);
        float av[4], bv[4], z[4], xv[4], tv[4];
        load_group<VEC>(x0 + i, count, av);
        load_group<VEC>(y + i, count, bv);
        philox_normal4(seed, ordinal, BBDM_NOISE_Q_SAMPLE, q, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const QSample r = q_sample_one(objective, m, sig, av[j], bv[j], z[j]);
            xv[j] = r.x_t;
            tv[j] = r.target;
        }
        store_group<VEC>(x_t + i, count, xv);
        store_group<VEC>(target + i, count, tv);
    }
}

// ---- latent cache (bbdm_amd/latent_cache.py): q_sample whose x0 / y rows are GATHERED from two cache tensors of raw (un-normalised)
// latents, one image per blockIdx.y as above.  Replaces the two frozen-encoder passes of LatentBrownianBridgeModel.forward
// (LatentBrownianBridgeModel.py:68-72) and encode()'s normalisation (:92-97) in front of q_sample (BrownianBridgeModel.py:128-146).
// NORM: (z - mean[c]) / std[c], two separate fp32 operations with an IEEE division -- the operations torch performs for encode(); the
// channel of element e is e / hw, so an unaligned group of four may straddle two channels.  The q_sample expressions are
// q_sample_kernel's, in the same order.  An image whose index is outside [0, M) dereferences nothing and gets NaN in all three outputs.
// PHILOX: the noise of domain 1 in registers (noise unused), else the noise tensor (seed / ordinal unused).
template <bool VEC, bool PHILOX>
__global__ void __launch_bounds__(256) q_sample_cached_kernel(const float* __restrict__ ori, const float* __restrict__ cond, int64_t M,
                                                              const int64_t* __restrict__ idx_ori, const int64_t* __restrict__ idx_cond,
                                                              const float* __restrict__ ori_mean, const float* __restrict__ ori_std,
                                                              const float* __restrict__ cond_mean, const float* __restrict__ cond_std,
                                                              int hw, const float* __restrict__ noise,
                                                              const int64_t* __restrict__ seed_arr, const int64_t* __restrict__ ordinal_arr,
                                                              const int64_t* __restrict__ t, const float* __restrict__ m_t,
                                                              const float* __restrict__ var_t, float* __restrict__ x_t,
                                                              float* __restrict__ target, float* __restrict__ y_out, int per_sample,
                                                              int objective) {
    const int n = blockIdx.y;
    const int64_t io = idx_ori[n], ic = idx_cond[n];
    const size_t base = (size_t)n * per_sample;
    const unsigned groups = ((unsigned)per_sample + 3u) / 4u;
    if (io < 0 || io >= M || ic < 0 || ic >= M) {
        const float nan = __builtin_nanf("");
        const float bad[4] = {nan, nan, nan, nan};
        for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < groups; q += gridDim.x * 256u) {
            const size_t i = base + 4 * (size_t)q;
            const int count = per_sample - (int)(4u * q);
            store_group<VEC>(x_t + i, count, bad);
            store_group<VEC>(target + i, count, bad);
            store_group<VEC>(y_out + i, count, bad);
        }
        return;
    }
    const float* __restrict__ a_row = ori + (size_t)io * per_sample;
    const float* __restrict__ b_row = cond + (size_t)ic * per_sample;
    const int64_t tt = t[n];
    const float m = m_t[tt];
    const float sig = sqrtf(var_t[tt]);
    int64_t seed = 0, ordinal = 0;
    if (PHILOX) seed = seed_arr[n], ordinal = ordinal_arr[n];
    for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < groups; q += gridDim.x * 256u) {
        const size_t k = 4 * (size_t)q;
        const int count = per_sample - (int)(4u * q);
        float av[4], bv[4], z[4], xv[4], tv[4];
        load_group<VEC>(a_row + k, count, av);
        load_group<VEC>(b_row + k, count, bv);
        if (PHILOX) philox_normal4(seed, ordinal, BBDM_NOISE_Q_SAMPLE, q, z);
        else load_group<VEC>(noise + base + k, count, z);
        if (ori_mean) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < count) {                                   // (the tail's elements have no channel)
                    const int c = (int)((4u * q + (unsigned)j) / (unsigned)hw);
                    av[j] = (av[j] - ori_mean[c]) / ori_std[c];
                    bv[j] = (bv[j] - cond_mean[c]) / cond_std[c];
                }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const QSample r = q_sample_one(objective, m, sig, av[j], bv[j], z[j]);
            xv[j] = r.x_t;
            tv[j] = r.target;
        }
        store_group<VEC>(x_t + base + k, count, xv);
        store_group<VEC>(target + base + k, count, tv);
        store_group<VEC>(y_out + base + k, count, bv);
    }
}

// Per-channel sums over all M rows of one cache tensor [M, C, hw] -- the mean / variance loops of BBDMRunner.get_latent_mean_std
// (BBDMRunner.py:85-162).  SQ = false: sum of z into cells[c]; SQ = true: sum of (z - mean_f32[c])^2 into cells[C + c], mean_f32 re-derived
// from cells[c] by every block (the first launch has finished: same stream).  One (row, channel) plane per block iteration: every thread
// sums its groups of four in fp64 in a fixed order, the block reduces in a fixed tree, and the plane's partial goes into the exact limb
// cell (stats_acc.h).  The partial is a function of the plane's values alone (the same tree with 128-bit and with element accesses, the
// block size is fixed) and the limbs add associatively, so the sums are a function of the MULTISET of rows: not of their order, and not
// of how many blocks share them.  A non-finite partial bumps the cell's fourth word: that channel reads NaN.
template <bool VEC, bool SQ>
__global__ void __launch_bounds__(256) latent_stats_kernel(const float* __restrict__ z, int64_t M, int C, int hw,
                                                           unsigned long long* __restrict__ cells, double count) {
    const int c = blockIdx.y;
    double mean = 0.0;
    if (SQ) mean = (double)(float)(sa_load(cells + (size_t)c * SA_W) / count);
    unsigned long long* cell = cells + ((size_t)(SQ ? C : 0) + c) * SA_W;
    const int groups = (hw + 3) / 4;
    for (int64_t r = blockIdx.x; r < M; r += gridDim.x) {
        const float* __restrict__ p = z + ((size_t)r * C + c) * hw;
        double s = 0.0;
        for (int q = threadIdx.x; q < groups; q += 256) {
            const int cnt = hw - 4 * q;
            float v[4];
            load_group<VEC>(p + 4 * (size_t)q, cnt, v);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) {
                    const double d = (double)v[j] - mean;
                    s += SQ ? d * d : d;
                }
        }
        const double total = block_sum_down(s);
        if (threadIdx.x == 0) sa_add(cell, total);
        __syncthreads();                                   // block_sum_down's partials are rewritten by the next row
    }
}

__global__ void latent_stats_final_kernel(const unsigned long long* __restrict__ cells, int C, double count, float* __restrict__ mean,
                                          float* __restrict__ var, float* __restrict__ stdev) {
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < C; c += gridDim.x * blockDim.x) {
        const double v = sa_load(cells + ((size_t)C + c) * SA_W) / count;
        mean[c] = (float)(sa_load(cells + (size_t)c * SA_W) / count);
        var[c] = (float)v;
        stdev[c] = (float)sqrt(v);
    }
}

__global__ void __launch_bounds__(256) loss_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           unsigned long long* __restrict__ partial, size_t count, int loss_type) {
    double s = 0.0;
    for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) s += loss_term(a[i], b[i], loss_type);
    const double total = block_sum_down(s);
    if (threadIdx.x == 0) sa_add(partial, total);          // exact limb cell: any block order, same bits
}

__global__ void loss_final_kernel(const unsigned long long* __restrict__ partial, float* __restrict__ out, double inv_count) {
    out[0] = (float)(sa_load(partial) * inv_count);
}

// d loss / d pred (same NCHW layout as pred):  l1: sign(pred - target) / count ; l2: 2 (pred - target) / count ;
// times the upstream scalar gradient gscale[0] (read on the device: no host sync).
__global__ void loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                const float* __restrict__ gscale, float* __restrict__ dpred, size_t total,
                                float inv_count, int loss_type) {
    const float g = gscale[0] * inv_count;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const float d = pred[i] - target[i];
        dpred[i] = loss_type == 0 ? (d > 0.f ? g : (d < 0.f ? -g : 0.f)) : 2.f * d * g;
    }
}

// NCHW (a [+ b]) -> NHWC with zero channel padding.  One thread per output pixel-channel; reads are coalesced
// along w for each source plane (C is tiny here: 3..16), writes are contiguous.
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ a, int Ca, const float* __restrict__ b, int Cb,
                                    float* __restrict__ out, int ldo, int Cpad, int HW, size_t total) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cpad);
        const size_t pix = i / Cpad;
        const size_t n = pix / HW, p = pix - n * HW;
        float v = 0.f;
        if (c < Ca) v = a[(n * Ca + c) * HW + p];
        else if (c < Ca + Cb) v = b[(n * Cb + (c - Ca)) * HW + p];
        out[pix * ldo + c] = v;
    }
}

__global__ void nhwc_to_nchw_kernel(const float* __restrict__ x, int ldx, float* __restrict__ out, int C, int HW,
                                    size_t total) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i % HW;
        const size_t nc = i / HW;
        const size_t n = nc / C, c = nc - n * C;
        out[i] = x[(n * HW + p) * ldx + c];
    }
}

// The argument checks of a one-image-per-blockIdx.y launch (N is gridDim.y).  counter: the kernel numbers its groups of four in the
// 32-bit counter word of Philox.
int check_per_image(const char* what, int N, int per_sample, int objective, bool counter) {
    BBDM_REQUIRE(N > 0 && N <= 65535 && per_sample > 0 && objective >= 0 && objective <= 2, "%s: bad args", what);
    BBDM_REQUIRE(!counter || (unsigned long long)per_sample / 4 < (1ull << 32), "%s: per_sample / 4 must fit the 32-bit counter word", what);
    return BBDM_OK;
}

// The checks and the launch shared by the uniform and the per-request entry point of each per-image kernel (P as above).
template <class P>
int launch_p_step_batched(const char* what, const float* x_t, const float* y, const float* pred, const float* noise,
                          const float* m_t, const float* variance_t, const int64_t* t, const int64_t* t_next,
                          const int64_t* flag, P params, int objective, float* x_next, float* x0_recon, float* x_next_alias,
                          int N, int per_sample, void* stream) {
    BBDM_REQUIRE(x_t && y && pred && noise && m_t && variance_t && t && t_next && flag && x_next && x0_recon,
                 "%s: null pointer", what);
    if (const int rc = check_per_image(what, N, per_sample, objective, false)) return rc;
    const size_t b = ((size_t)per_sample + 255) / 256;
    const unsigned bx = (unsigned)(b > 2048 ? 2048 : b);
    hipLaunchKernelGGL(p_step_batched_kernel<P>, dim3(bx, (unsigned)N), dim3(256), 0, (hipStream_t)stream, x_t, y, pred, noise,
                       m_t, variance_t, t, t_next, flag, params, objective, x_next, x0_recon, x_next_alias, per_sample);
    BBDM_CHECK_LAUNCH(what);
    return BBDM_OK;
}

template <class P>
int launch_p_step_philox(const char* what, const float* x_t, const float* y, const float* pred, const int64_t* seed,
                         const int64_t* ordinal, const float* m_t, const float* variance_t, const int64_t* t,
                         const int64_t* t_next, const int64_t* flag, P params, int objective, float* x_next, float* x0_recon,
                         float* x_next_alias, int N, int per_sample, void* stream) {
    BBDM_REQUIRE(x_t && y && pred && seed && ordinal && m_t && variance_t && t && t_next && flag && x_next && x0_recon,
                 "%s: null pointer", what);
    if (const int rc = check_per_image(what, N, per_sample, objective, true)) return rc;
    const bool vec = per_sample % 4 == 0 && aligned16(x_t) && aligned16(y) && aligned16(pred) && aligned16(x_next) &&
                     aligned16(x0_recon) && aligned16(x_next_alias);
    return dispatch([&](auto VEC) {
        hipLaunchKernelGGL((p_step_philox_kernel<VEC(), P>), group_grid(N, per_sample), dim3(256), 0, (hipStream_t)stream, x_t, y, pred,
                           seed, ordinal, m_t, variance_t, t, t_next, flag, params, objective, x_next, x0_recon, x_next_alias, per_sample);
        BBDM_CHECK_LAUNCH(what);
        return BBDM_OK;
    }, vec);
}

// The checks and the launch shared by the two cached q_sample entry points (PHILOX as in the kernel).
template <bool PHILOX>
int launch_q_sample_cached(const char* what, const float* ori, const float* cond, long long M, const int64_t* idx_ori,
                           const int64_t* idx_cond, const float* ori_mean, const float* ori_std, const float* cond_mean,
                           const float* cond_std, int hw, const float* noise, const int64_t* seed, const int64_t* ordinal,
                           const int64_t* t, const float* m_t, const float* variance_t, float* x_t, float* target, float* y_out, int N,
                           int per_sample, int objective, void* stream) {
    BBDM_REQUIRE(ori && cond && idx_ori && idx_cond && t && m_t && variance_t && x_t && target && y_out, "%s: null pointer", what);
    BBDM_REQUIRE(PHILOX ? (seed && ordinal) : noise != nullptr, "%s: null noise source", what);
    const int stats = (ori_mean != nullptr) + (ori_std != nullptr) + (cond_mean != nullptr) + (cond_std != nullptr);
    BBDM_REQUIRE(stats == 0 || stats == 4, "%s: pass all four of ori_mean / ori_std / cond_mean / cond_std or none", what);
    BBDM_REQUIRE(M > 0, "%s: bad args", what);
    if (const int rc = check_per_image(what, N, per_sample, objective, true)) return rc;
    BBDM_REQUIRE(hw > 0 && per_sample % hw == 0, "%s: per_sample must be a multiple of hw", what);
    // (per_sample % 4 == 0 makes every gathered row as aligned as its tensor)
    const bool vec = per_sample % 4 == 0 && aligned16(ori) && aligned16(cond) && aligned16(noise) && aligned16(x_t) &&
                     aligned16(target) && aligned16(y_out);
    return dispatch([&](auto VEC) {
        hipLaunchKernelGGL((q_sample_cached_kernel<VEC(), PHILOX>), group_grid(N, per_sample), dim3(256), 0, (hipStream_t)stream, ori, cond,
                           (int64_t)M, idx_ori, idx_cond, ori_mean, ori_std, cond_mean, cond_std, hw, noise, seed, ordinal, t, m_t,
                           variance_t, x_t, target, y_out, per_sample, objective);
        BBDM_CHECK_LAUNCH(what);
        return BBDM_OK;
    }, vec);
}

}  // namespace

extern "C" int bbdm_bb_q_sample_f32(const float* x0, const float* y, const float* noise, const int64_t* t,
                                    const float* m_t, const float* variance_t, float* x_t, float* target, int N,
                                    int per_sample, int objective, void* stream) {
    BBDM_REQUIRE(x0 && y && noise && t && m_t && variance_t && x_t && target, "q_sample: null pointer");
    BBDM_REQUIRE(N > 0 && per_sample > 0 && objective >= 0 && objective <= 2, "q_sample: bad args");
    const size_t total = (size_t)N * per_sample;
    hipLaunchKernelGGL(q_sample_kernel, dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)stream, x0, y, noise, t, m_t,
                       variance_t, x_t, target, per_sample, total, objective);
    BBDM_CHECK_LAUNCH("q_sample");
    return BBDM_OK;
}

extern "C" int bbdm_bb_predict_x0_f32(const float* x_t, const float* y, const float* pred, const int64_t* t,
                                      const float* m_t, const float* variance_t, float* x0_recon, int N,
                                      int per_sample, int objective, void* stream) {
    BBDM_REQUIRE(x_t && y && pred && t && m_t && variance_t && x0_recon, "predict_x0: null pointer");
    BBDM_REQUIRE(N > 0 && per_sample > 0 && objective >= 0 && objective <= 2, "predict_x0: bad args");
    const size_t total = (size_t)N * per_sample;
    hipLaunchKernelGGL(predict_x0_kernel, dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)stream, x_t, y, pred, t,
                       m_t, variance_t, x0_recon, per_sample, total, objective);
    BBDM_CHECK_LAUNCH("predict_x0");
    return BBDM_OK;
}

extern "C" int bbdm_bb_p_sample_step_f32(const float* x_t, const float* y, const float* pred, const float* noise,
                                         const float* m_t, const float* variance_t, int t, int t_next, int is_last,
                                         float eta, int clip, int objective, float* x_next, float* x0_recon,
                                         float* x_next_alias, int N, int per_sample, void* stream) {
    BBDM_REQUIRE(x_t && y && pred && m_t && variance_t && x_next && x0_recon, "p_sample_step: null pointer");
    BBDM_REQUIRE(is_last || noise, "p_sample_step: noise required unless is_last");
    BBDM_REQUIRE(N > 0 && per_sample > 0 && objective >= 0 && objective <= 2 && t >= 0 && (is_last || t_next >= 0),
                 "p_sample_step: bad args");
    const size_t total = (size_t)N * per_sample;
    hipLaunchKernelGGL(p_step_kernel, dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)stream, x_t, y, pred, noise,
                       m_t, variance_t, t, t_next, is_last, eta, clip, objective, x_next, x0_recon, x_next_alias, total);
    BBDM_CHECK_LAUNCH("p_sample_step");
    return BBDM_OK;
}

extern "C" int bbdm_bb_p_sample_step_batched_f32(const float* x_t, const float* y, const float* pred, const float* noise,
                                                 const float* m_t, const float* variance_t, const int64_t* t,
                                                 const int64_t* t_next, const int64_t* flag, float eta, int clip, int objective,
                                                 float* x_next, float* x0_recon, float* x_next_alias, int N, int per_sample,
                                                 void* stream) {
    return launch_p_step_batched("p_sample_step_batched", x_t, y, pred, noise, m_t, variance_t, t, t_next, flag,
                                 UniformParams{eta, clip}, objective, x_next, x0_recon, x_next_alias, N, per_sample, stream);
}

extern "C" int bbdm_bb_p_sample_step_requests_f32(const float* x_t, const float* y, const float* pred, const float* noise,
                                                  const float* m_t, const float* variance_t, const int64_t* t,
                                                  const int64_t* t_next, const int64_t* flag, const float* eta, int objective,
                                                  float* x_next, float* x0_recon, float* x_next_alias, int N, int per_sample,
                                                  void* stream) {
    BBDM_REQUIRE(eta, "p_sample_step_requests: null eta");
    return launch_p_step_batched("p_sample_step_requests", x_t, y, pred, noise, m_t, variance_t, t, t_next, flag,
                                 RequestParams{eta}, objective, x_next, x0_recon, x_next_alias, N, per_sample, stream);
}

extern "C" int bbdm_philox_normal_f32(float* out, const int64_t* seed, const int64_t* ordinal, int domain, int N,
                                      int per_sample, void* stream) {
    BBDM_REQUIRE(out && seed && ordinal, "philox_normal: null pointer");
    BBDM_REQUIRE(domain >= 0, "philox_normal: bad args");
    if (const int rc = check_per_image("philox_normal", N, per_sample, 0, true)) return rc;
    return dispatch([&](auto VEC) {
        hipLaunchKernelGGL(philox_normal_kernel<VEC()>, group_grid(N, per_sample), dim3(256), 0, (hipStream_t)stream, out, seed, ordinal,
                           (unsigned)domain, per_sample);
        BBDM_CHECK_LAUNCH("philox_normal");
        return BBDM_OK;
    }, per_sample % 4 == 0 && aligned16(out));
}

extern "C" int bbdm_philox_raw_u32(const uint32_t* counter_key, uint32_t* out, int n, void* stream) {
    BBDM_REQUIRE(counter_key && out && n > 0, "philox_raw: bad args");
    hipLaunchKernelGGL(philox_raw_kernel, dim3(ew_blocks((size_t)n)), dim3(256), 0, (hipStream_t)stream, counter_key, out, n);
    BBDM_CHECK_LAUNCH("philox_raw");
    return BBDM_OK;
}

extern "C" int bbdm_bb_p_sample_step_philox_f32(const float* x_t, const float* y, const float* pred, const int64_t* seed,
                                                const int64_t* ordinal, const float* m_t, const float* variance_t,
                                                const int64_t* t, const int64_t* t_next, const int64_t* flag, float eta,
                                                int clip, int objective, float* x_next, float* x0_recon, float* x_next_alias,
                                                int N, int per_sample, void* stream) {
    return launch_p_step_philox("p_sample_step_philox", x_t, y, pred, seed, ordinal, m_t, variance_t, t, t_next, flag,
                                UniformParams{eta, clip}, objective, x_next, x0_recon, x_next_alias, N, per_sample, stream);
}

extern "C" int bbdm_bb_p_sample_step_requests_philox_f32(const float* x_t, const float* y, const float* pred,
                                                         const int64_t* seed, const int64_t* ordinal, const float* m_t,
                                                         const float* variance_t, const int64_t* t, const int64_t* t_next,
                                                         const int64_t* flag, const float* eta, int objective, float* x_next,
                                                         float* x0_recon, float* x_next_alias, int N, int per_sample,
                                                         void* stream) {
    BBDM_REQUIRE(eta, "p_sample_step_requests_philox: null eta");
    return launch_p_step_philox("p_sample_step_requests_philox", x_t, y, pred, seed, ordinal, m_t, variance_t, t, t_next, flag,
                                RequestParams{eta}, objective, x_next, x0_recon, x_next_alias, N, per_sample, stream);
}

extern "C" int bbdm_bb_q_sample_philox_f32(const float* x0, const float* y, const int64_t* seed, const int64_t* ordinal,
                                           const int64_t* t, const float* m_t, const float* variance_t, float* x_t,
                                           float* target, int N, int per_sample, int objective, void* stream) {
    BBDM_REQUIRE(x0 && y && seed && ordinal && t && m_t && variance_t && x_t && target, "q_sample_philox: null pointer");
    if (const int rc = check_per_image("q_sample_philox", N, per_sample, objective, true)) return rc;
    return dispatch([&](auto VEC) {
        hipLaunchKernelGGL(q_sample_philox_kernel<VEC()>, group_grid(N, per_sample), dim3(256), 0, (hipStream_t)stream, x0, y, seed,
                           ordinal, t, m_t, variance_t, x_t, target, per_sample, objective);
        BBDM_CHECK_LAUNCH("q_sample_philox");
        return BBDM_OK;
    }, per_sample % 4 == 0 && aligned16(x0) && aligned16(y) && aligned16(x_t) && aligned16(target));
}

extern "C" int bbdm_bb_q_sample_cached_f32(const float* ori, const float* cond, long long M, const int64_t* idx_ori,
                                           const int64_t* idx_cond, const float* ori_mean, const float* ori_std,
                                           const float* cond_mean, const float* cond_std, int hw, const float* noise,
                                           const int64_t* t, const float* m_t, const float* variance_t, float* x_t, float* target,
                                           float* y_out, int N, int per_sample, int objective, void* stream) {
    return launch_q_sample_cached<false>("q_sample_cached", ori, cond, M, idx_ori, idx_cond, ori_mean, ori_std, cond_mean, cond_std,
                                         hw, noise, nullptr, nullptr, t, m_t, variance_t, x_t, target, y_out, N, per_sample, objective,
                                         stream);
}

extern "C" int bbdm_bb_q_sample_cached_philox_f32(const float* ori, const float* cond, long long M, const int64_t* idx_ori,
                                                  const int64_t* idx_cond, const float* ori_mean, const float* ori_std,
                                                  const float* cond_mean, const float* cond_std, int hw, const int64_t* seed,
                                                  const int64_t* ordinal, const int64_t* t, const float* m_t,
                                                  const float* variance_t, float* x_t, float* target, float* y_out, int N,
                                                  int per_sample, int objective, void* stream) {
    return launch_q_sample_cached<true>("q_sample_cached_philox", ori, cond, M, idx_ori, idx_cond, ori_mean, ori_std, cond_mean,
                                        cond_std, hw, nullptr, seed, ordinal, t, m_t, variance_t, x_t, target, y_out, N, per_sample,
                                        objective, stream);
}

extern "C" int bbdm_latent_channel_stats_f32(const float* z, long long M, int C, int hw, double* cells, float* mean, float* var,
                                             float* stdev, int row_blocks, void* stream) {
    BBDM_REQUIRE(z && cells && mean && var && stdev, "latent_channel_stats: null pointer");
    // one sa_add per (row, channel) and pass: a limb has 23 spare bits (stats_acc.h)
    BBDM_REQUIRE(M > 0 && M < (1ll << 23) && C > 0 && C <= 65535 && hw > 0 && row_blocks >= 0, "latent_channel_stats: bad args");
    unsigned long long* cell = reinterpret_cast<unsigned long long*>(cells);     // [2][C] cells of 4 x 8 bytes, zeroed by the caller
    const long long want = row_blocks ? row_blocks : 1024;
    const dim3 grid((unsigned)(want < M ? want : M), (unsigned)C);
    const double count = (double)M * (double)hw;
    const bool vec = hw % 4 == 0 && aligned16(z);
    const auto pass = [&](auto VEC, auto SQ) {              // SQ: the squared deviations from the mean the first pass gives
        hipLaunchKernelGGL((latent_stats_kernel<VEC(), SQ()>), grid, dim3(256), 0, (hipStream_t)stream, z, (int64_t)M, C, hw, cell, count);
        BBDM_CHECK_LAUNCH("latent_channel_stats");
        return BBDM_OK;
    };
    if (const int rc = dispatch(pass, vec, false)) return rc;
    if (const int rc = dispatch(pass, vec, true)) return rc;
    hipLaunchKernelGGL(latent_stats_final_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cell, C, count,
                       mean, var, stdev);
    BBDM_CHECK_LAUNCH("latent_channel_stats");
    return BBDM_OK;
}

extern "C" int bbdm_bb_loss_f32(const float* a, const float* b, double* partial, float* out, size_t count,
                                int loss_type, void* stream) {
    BBDM_REQUIRE(a && b && partial && out && count > 0 && (loss_type == 0 || loss_type == 1), "loss: bad args");
    size_t blocks = (count + 256 * 8 - 1) / (256 * 8);
    if (blocks > 1024) blocks = 1024;
    unsigned long long* cell = reinterpret_cast<unsigned long long*>(partial);     // 4 x 8 bytes (stats_acc.h), zeroed by the caller
    hipLaunchKernelGGL(loss_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, cell,
                       count, loss_type);
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, cell, out, 1.0 / (double)count);
    BBDM_CHECK_LAUNCH("loss");
    return BBDM_OK;
}

extern "C" int bbdm_bb_loss_bwd_f32(const float* pred, const float* target, const float* gscale, float* dpred,
                                    size_t count, int loss_type, void* stream) {
    BBDM_REQUIRE(pred && target && gscale && dpred && count > 0 && (loss_type == 0 || loss_type == 1),
                 "loss_bwd: bad args");
    hipLaunchKernelGGL(loss_bwd_kernel, dim3(ew_blocks(count)), dim3(256), 0, (hipStream_t)stream, pred, target, gscale,
                       dpred, count, 1.0f / (float)count, loss_type);
    BBDM_CHECK_LAUNCH("loss_bwd");
    return BBDM_OK;
}

extern "C" int bbdm_nchw_to_nhwc_f32(const float* a, int Ca, const float* b, int Cb, float* out, int ldo, int Cpad,
                                     int N, int H, int W, void* stream) {
    BBDM_REQUIRE(a && out && Ca > 0 && Cb >= 0 && (Cb == 0 || b), "nchw_to_nhwc: bad args");
    BBDM_REQUIRE(Cpad >= Ca + Cb && ldo >= Cpad && N > 0 && H > 0 && W > 0, "nchw_to_nhwc: bad shape");
    const size_t total = (size_t)N * H * W * Cpad;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)stream, a, Ca, b, Cb, out,
                       ldo, Cpad, H * W, total);
    BBDM_CHECK_LAUNCH("nchw_to_nhwc");
    return BBDM_OK;
}

extern "C" int bbdm_nhwc_to_nchw_f32(const float* x, int ldx, float* out, int N, int H, int W, int C, void* stream) {
    BBDM_REQUIRE(x && out && N > 0 && H > 0 && W > 0 && C > 0 && ldx >= C, "nhwc_to_nchw: bad args");
    const size_t total = (size_t)N * H * W * C;
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)stream, x, ldx, out, C,
                       H * W, total);
    BBDM_CHECK_LAUNCH("nhwc_to_nchw");
    return BBDM_OK;
}
