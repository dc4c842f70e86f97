// optim.hip -- the optimizer side of the training step as ONE HBM-bound pass.
//
// Replaces, per optimizer step of the 237 M-parameter UNet (248 tensors):
//   * torch.optim.Adam.step()  (runners/utils.py:48-51: Adam(lr, weight_decay, betas=(beta1, 0.999)), eps 1e-8, no amsgrad)
//     -- ~10 ATen foreach kernels over p, g, m, v in the reference's torch 1.12 (``_single_tensor_adam``: 248 x ~8 launches);
//   * EMA.update()             (runners/base/EMA.py:21-29: shadow = (1 - d) * p + d * shadow, or shadow = p before
//     start_ema_step) -- 248 x 4 launches + a clone each;
// with one launch over a table of (param, grad, exp_avg, exp_avg_sq, shadow) chunks: p, g, m, v are read once and p, m, v
// (and the EMA shadow, when due) written once: 7 (+2) x 4 B per parameter = 6.6 (8.5) GB per step at 237 M parameters.
// The tensors stay where torch put them (leaf nn.Parameters, .grad views of the backward plan's flat buffer or DDP bucket
// views): the table holds raw pointers, so no flattening / re-pointing of parameters is needed.
//
// Arithmetic follows the single-tensor path of torch.optim.Adam in torch >= 2.0 operation by operation (this file is built with
// -ffp-contract=off, like bridge.hip) -- the torch the tests compare with.  The reference's torch 1.12 updates the first moment as
// exp_avg.mul_(beta1).add_(grad, alpha=1 - beta1): the same value up to one fp32 rounding per step, not bit for bit.
//     g' = g + wd * p                                  (weight_decay != 0)
//     m  = lerp(m, g', 1 - b1)                         (exp_avg.lerp_(grad, 1 - beta1); at::lerp's two-branch formula)
//     v  = v * b2 + (1 - b2) * g' * g'                 (exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2))
//     p  = p - (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps)),   bc1 = 1 - b1^step, bc2 = 1 - b2^step  (host doubles -> fp32)
//
// Global L2 gradient-norm clipping + non-finite guard (ABI 28; torch.nn.utils.clip_grad_norm_ in front of the step, no host read-back):
//   grad_sqnorm_kernel   one workgroup per chunk of the SAME table: sum g^2 in fp64 in a fixed order -- thread t adds the float4 groups
//                        t, t + 256, ... of the chunk serially (then tail element t), a 64-lane butterfly and a fixed 4-wave sum follow;
//                        the element -> thread assignment does not depend on the alignment of the pointer.  The chunk's partial, times
//                        2^18, is added to cell (workgroup % 256) as integer limbs (stats_acc.h: sa_add).  Integer limbs add exactly, so
//                        WHICH cell a partial lands in is immaterial: the reader adds the 256 cells limb by limb as integers and folds
//                        once.  The norm is a function of the gradient values and the chunk boundaries only -- not of the grid, the order
//                        in which workgroups finish, the order of the table's rows, or the number of tables.  The cells (one per 128-byte
//                        line) only keep the ~14 500 workgroups of the full model from meeting on ONE address (~57
//                        adds per cell instead).
//                        WINDOW: sa_add takes |v| < 2^50 at a resolution of 2^-70; with the 2^18 pre-scale a chunk's sum of squares must
//                        be < 2^32 (chunk norm < 65 536) and is truncated at 2^-88.  14 500 truncations are <= 4.7e-23 of the squared
//                        norm: a relative error of 2.4e-7 for a total norm of 1e-8, less above (+ 6e-8: the fp32 rounding of the
//                        output).  A chunk outside the window, or a non-finite one, bumps the cell's fourth word: the norm is NaN --
//                        where torch's would be Inf (an Inf gradient) or a finite number > 65 536.
//   grad_finalize_kernel one workgroup: norm, coef = min(1, (1 / (norm + 1e-6)) * max_norm) in fp32 as torch forms it (NaN stays NaN), ok, and
//                        the device counter of skipped steps.
//   adam_ema_kernel<true> g * coef (one rounding, as grads.mul_(coef)) in front of adam_one; ok == 0 under skip_nonfinite: no Adam update
//                        (the EMA part still runs, as the runner's ema.update would).
//   grad_scale_kernel    g *= coef (the standalone clip_grad_norm_).
//   rule_ema_kernel      the SGD and RMSprop rules (runners/utils.py:52-55) with the same mapping, clip buffer and EMA part: below.
#include "common.h"
#include "stats_acc.h"

namespace {

constexpr int CHUNK = 16384;       // elements per table entry = per workgroup (64 per thread)

struct OptArgs {
    const BbdmOptChunk* table;
    float lr_over_bc1, sqrt_bc2, b1c, b2, b2c, eps, wd;     // b1c = 1 - beta1, b2c = 1 - beta2
    float ema_decay, ema_c;                                       // ema_c = 1 - decay
    int do_adam, ema_mode;                                        // ema_mode: 0 none, 1 decay, 2 copy
    const float* clip;                                            // adam_ema_kernel<true>: {norm, coef, ok, 0} of grad_finalize_kernel
    int skip_nonfinite;
};

__device__ __forceinline__ void adam_one(const OptArgs& a, float& p, float g, float& m, float& v) {
    if (a.wd != 0.f) g = fmaf(a.wd, p, g);          // grad.add(param, alpha=wd): one rounding in ATen's kernels
    // at::lerp: |w| < 0.5 ? a + w (b - a) : b - (b - a) (1 - w),  w = 1 - beta1
    m = a.b1c < 0.5f ? m + a.b1c * (g - m) : g - (g - m) * (1.f - a.b1c);
    v = v * a.b2 + a.b2c * g * g;
    const float denom = sqrtf(v) / a.sqrt_bc2 + a.eps;
    p = p - a.lr_over_bc1 * (m / denom);
}

// CLIP = false is bbdm_adam_ema_step_f32, instruction for instruction what it was before the clipped entry point existed
template <bool CLIP>
__global__ void __launch_bounds__(256) adam_ema_kernel(const OptArgs a) {
    const BbdmOptChunk c = a.table[blockIdx.x];
    float* __restrict__ p = c.param;
    const float* __restrict__ g = c.grad;
    float* __restrict__ m = c.exp_avg;
    float* __restrict__ v = c.exp_avg_sq;
    float* __restrict__ s = c.shadow;
    const int n = c.n;
    bool adam = a.do_adam && g != nullptr;            // a parameter without a gradient is skipped, as torch does
    float coef = 1.f;
    if (CLIP) {
        coef = a.clip[1];
        if (a.skip_nonfinite && a.clip[2] == 0.f) adam = false;      // non-finite norm: p, m, v stay as they are
    }
    const bool ema = a.ema_mode != 0 && s != nullptr;
    const uintptr_t al = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)s;
    if ((al & 15) == 0) {
        const int n4 = n >> 2;
        for (int i = threadIdx.x; i < n4; i += 256) {
            float4 pv = reinterpret_cast<const float4*>(p)[i];
            if (adam) {
                float4 gv = reinterpret_cast<const float4*>(g)[i];
                if (CLIP) { gv.x *= coef; gv.y *= coef; gv.z *= coef; gv.w *= coef; }
                float4 mv = reinterpret_cast<const float4*>(m)[i];
                float4 vv = reinterpret_cast<const float4*>(v)[i];
                adam_one(a, pv.x, gv.x, mv.x, vv.x);
                adam_one(a, pv.y, gv.y, mv.y, vv.y);
                adam_one(a, pv.z, gv.z, mv.z, vv.z);
                adam_one(a, pv.w, gv.w, mv.w, vv.w);
                reinterpret_cast<float4*>(m)[i] = mv;
                reinterpret_cast<float4*>(v)[i] = vv;
                reinterpret_cast<float4*>(p)[i] = pv;
            }
            if (ema) {
                float4 sv = pv;
                if (a.ema_mode == 1) {
                    const float4 o = reinterpret_cast<const float4*>(s)[i];
                    sv.x = a.ema_c * pv.x + a.ema_decay * o.x;
                    sv.y = a.ema_c * pv.y + a.ema_decay * o.y;
                    sv.z = a.ema_c * pv.z + a.ema_decay * o.z;
                    sv.w = a.ema_c * pv.w + a.ema_decay * o.w;
                }
                reinterpret_cast<float4*>(s)[i] = sv;
            }
        }
        for (int i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
            float pv = p[i];
            if (adam) {
                float mv = m[i], vv = v[i];
                adam_one(a, pv, CLIP ? g[i] * coef : g[i], mv, vv);
                m[i] = mv; v[i] = vv; p[i] = pv;
            }
            if (ema) s[i] = a.ema_mode == 1 ? a.ema_c * pv + a.ema_decay * s[i] : pv;
        }
    } else {
        for (int i = threadIdx.x; i < n; i += 256) {
            float pv = p[i];
            if (adam) {
                float mv = m[i], vv = v[i];
                adam_one(a, pv, CLIP ? g[i] * coef : g[i], mv, vv);
                m[i] = mv; v[i] = vv; p[i] = pv;
            }
            if (ema) s[i] = a.ema_mode == 1 ? a.ema_c * pv + a.ema_decay * s[i] : pv;
        }
    }
}

// ---- the two other update rules of runners/utils.py:48-57 (RMSProp, SGD) on the same chunk table (ABI 30) ----------------------------
// torch's single-tensor formulas (_single_tensor_sgd / _single_tensor_rmsprop), operation by operation.  An add with a Python-number
// alpha (grad.add(param, alpha=wd), buf.add_(grad, alpha=1 - dampening), param.add_(grad, alpha=-lr)) is ONE rounding in ATen's CPU
// kernels: fmaf here, as adam_one does for the weight decay; addcmul / addcdiv are written as adam_one writes them.
//   SGD      g' = g + wd * p;  buf = first ? g' : momentum * buf + (1 - dampening) * g';  g' = nesterov ? g' + momentum * buf : buf;
//            p = p - lr * g'                                                  (the buf lines only with momentum != 0)
//   RMSprop  g' = g + wd * p;  sq = alpha * sq + (1 - alpha) * g' * g';  avg = sqrt(sq) + eps;
//            momentum != 0: buf = momentum * buf + g' / avg, p = p - lr * buf;  else p = p - lr * (g' / avg)
// The table's exp_avg slot carries the momentum buffer (NULL without momentum), the exp_avg_sq slot RMSprop's square_avg (NULL for SGD).
enum { RULE_SGD = 0, RULE_RMSPROP = 1 };

struct RuleArgs {
    const BbdmOptChunk* table;
    float lr, wd, mom, damp_c, alpha, alpha_c, eps;              // damp_c = 1 - dampening, alpha_c = 1 - alpha
    float ema_decay, ema_c;
    int nesterov, first, ema_mode;                                // first: SGD's first step with momentum: buf = g' (buf is not read)
    const float* clip;                                            // rule_ema_kernel<.., .., true>: {norm, coef, ok, 0}
    int skip_nonfinite;
};

template <int RULE, bool MOM>
__device__ __forceinline__ void rule_one(const RuleArgs& a, float& p, float g, float& buf, float& sq) {
    if (a.wd != 0.f) g = fmaf(a.wd, p, g);
    if (RULE == RULE_SGD) {
        if (MOM) {
            buf = a.first ? g : fmaf(a.damp_c, g, a.mom * buf);
            g = a.nesterov ? fmaf(a.mom, buf, g) : buf;
        }
        p = fmaf(-a.lr, g, p);
    } else {
        sq = sq * a.alpha + a.alpha_c * g * g;
        const float avg = sqrtf(sq) + a.eps;
        if (MOM) {
            buf = a.mom * buf + g / avg;
            p = fmaf(-a.lr, buf, p);
        } else {
            p = p - a.lr * (g / avg);
        }
    }
}

// adam_ema_kernel's mapping and access widths; MOM: the rule reads / writes the momentum buffer, RULE_RMSPROP: square_avg.  A chunk
// whose gradient, or a state tensor the rule needs, is NULL gets no update (its EMA part still runs).
template <int RULE, bool MOM, bool CLIP>
__global__ void __launch_bounds__(256) rule_ema_kernel(const RuleArgs a) {
    constexpr bool SQ = RULE == RULE_RMSPROP;
    const BbdmOptChunk c = a.table[blockIdx.x];
    float* __restrict__ p = c.param;
    const float* __restrict__ g = c.grad;
    float* __restrict__ m = c.exp_avg;
    float* __restrict__ v = c.exp_avg_sq;
    float* __restrict__ s = c.shadow;
    const int n = c.n;
    bool upd = g != nullptr && (!MOM || m != nullptr) && (!SQ || v != nullptr);
    float coef = 1.f;
    if (CLIP) {
        coef = a.clip[1];
        if (a.skip_nonfinite && a.clip[2] == 0.f) upd = false;       // non-finite norm: p and the state stay as they are
    }
    const bool ema = a.ema_mode != 0 && s != nullptr;
    const bool rd_m = MOM && !(RULE == RULE_SGD && a.first);
    uintptr_t al = (uintptr_t)p | (uintptr_t)g | (uintptr_t)s;
    if (MOM) al |= (uintptr_t)m;
    if (SQ) al |= (uintptr_t)v;
    if ((al & 15) == 0) {
        const int n4 = n >> 2;
        for (int i = threadIdx.x; i < n4; i += 256) {
            float4 pv = reinterpret_cast<const float4*>(p)[i];
            if (upd) {
                float4 gv = reinterpret_cast<const float4*>(g)[i];
                if (CLIP) { gv.x *= coef; gv.y *= coef; gv.z *= coef; gv.w *= coef; }
                float4 mv = make_float4(0.f, 0.f, 0.f, 0.f), vv = mv;
                if (rd_m) mv = reinterpret_cast<const float4*>(m)[i];
                if (SQ) vv = reinterpret_cast<const float4*>(v)[i];
                rule_one<RULE, MOM>(a, pv.x, gv.x, mv.x, vv.x);
                rule_one<RULE, MOM>(a, pv.y, gv.y, mv.y, vv.y);
                rule_one<RULE, MOM>(a, pv.z, gv.z, mv.z, vv.z);
                rule_one<RULE, MOM>(a, pv.w, gv.w, mv.w, vv.w);
                if (MOM) reinterpret_cast<float4*>(m)[i] = mv;
                if (SQ) reinterpret_cast<float4*>(v)[i] = vv;
                reinterpret_cast<float4*>(p)[i] = pv;
            }
            if (ema) {
                float4 sv = pv;
                if (a.ema_mode == 1) {
                    const float4 o = reinterpret_cast<const float4*>(s)[i];
                    sv.x = a.ema_c * pv.x + a.ema_decay * o.x;
                    sv.y = a.ema_c * pv.y + a.ema_decay * o.y;
                    sv.z = a.ema_c * pv.z + a.ema_decay * o.z;
                    sv.w = a.ema_c * pv.w + a.ema_decay * o.w;
                }
                reinterpret_cast<float4*>(s)[i] = sv;
            }
        }
    }
    // element accesses: the tail of an aligned chunk, or all of an unaligned one
    for (int i = ((al & 15) == 0 ? (n >> 2) << 2 : 0) + threadIdx.x; i < n; i += 256) {
        float pv = p[i];
        if (upd) {
            float mv = rd_m ? m[i] : 0.f, vv = SQ ? v[i] : 0.f;
            rule_one<RULE, MOM>(a, pv, CLIP ? g[i] * coef : g[i], mv, vv);
            if (MOM) m[i] = mv;
            if (SQ) v[i] = vv;
            p[i] = pv;
        }
        if (ema) s[i] = a.ema_mode == 1 ? a.ema_c * pv + a.ema_decay * s[i] : pv;
    }
}

constexpr int NORM_CELLS = 256;          // accumulator cells of the squared norm, one per 128-byte line
constexpr int NORM_CELL_WORDS = 16;      // 64-bit words from one cell to the next (the first SA_W are used)
constexpr double NORM_PRESCALE = 0x1p18, NORM_UNSCALE = 0x1p-18;

// sum over the workgroup's 256 threads in a fixed order (butterfly inside each wave: a + b == b + a bit for bit, so every lane ends with
// the same value; then (w0 + w1) + (w2 + w3)); the result is valid in thread 0
__device__ __forceinline__ double block_sum_fixed(double v) {
    __shared__ double wave_sum[4];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
    __syncthreads();
    return (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

__global__ void __launch_bounds__(256) grad_sqnorm_kernel(const BbdmOptChunk* __restrict__ table, unsigned long long* __restrict__ cells) {
    const BbdmOptChunk c = table[blockIdx.x];
    const float* __restrict__ g = c.grad;
    if (g == nullptr) return;                          // wave-uniform: a parameter without a gradient is not part of the norm, as in torch
    const int n = c.n, n4 = n >> 2;
    double acc = 0.0;                                  // g * g is exact in fp64 (24 x 24 bits); one rounding per addition
    if (((uintptr_t)g & 15) == 0) {
#pragma unroll 4
        for (int i = threadIdx.x; i < n4; i += 256) {
            const float4 v = reinterpret_cast<const float4*>(g)[i];
            acc += (double)v.x * (double)v.x;
            acc += (double)v.y * (double)v.y;
            acc += (double)v.z * (double)v.z;
            acc += (double)v.w * (double)v.w;
        }
    } else {                                           // the same elements in the same order, read one by one
        for (int i = threadIdx.x; i < n4; i += 256) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double x = (double)g[4 * i + e];
                acc += x * x;
            }
        }
    }
    const int t = (n4 << 2) + threadIdx.x;
    if (t < n) acc += (double)g[t] * (double)g[t];
    const double total = block_sum_fixed(acc);
    if (threadIdx.x == 0) sa_add(cells + (size_t)(blockIdx.x % NORM_CELLS) * NORM_CELL_WORDS, total * NORM_PRESCALE);
}

__global__ void __launch_bounds__(NORM_CELLS) grad_finalize_kernel(const unsigned long long* __restrict__ cells, float max_norm,
                                                                  float* __restrict__ out, long long* __restrict__ skipped) {
    __shared__ unsigned long long w[SA_W][NORM_CELLS];
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < SA_W; ++k) w[k][t] = cells[(size_t)t * NORM_CELL_WORDS + k];
    __syncthreads();
    for (int d = NORM_CELLS / 2; d > 0; d >>= 1) {      // limbs add as integers: exact, so the shape of this tree does not matter
        if (t < d) {
#pragma unroll
            for (int k = 0; k < SA_W; ++k) w[k][t] += w[k][t + d];
        }
        __syncthreads();
    }
    if (t == 0) {
        const double sq = sa_fold(w[0][0], w[1][0], w[2][0], w[3][0]) * NORM_UNSCALE;
        const float norm = (float)sqrt(sq);
        const bool ok = fabsf(norm) <= 3.4028234664e38f;             // false for NaN and Inf
        // clip_coef = max_norm / (total_norm + 1e-6), which torch evaluates as (total_norm + 1e-6).reciprocal() * max_norm (Tensor.__rdiv__):
        // two fp32 roundings; clip_coef_clamped = clamp(clip_coef, max=1.0): NaN stays NaN.  max_norm = +inf: inf -> 1 (the norm is finite
        // and inside the window, so the reciprocal is > 0)
        const float q = (1.f / (norm + 1e-6f)) * max_norm;
        out[0] = norm;
        out[1] = q > 1.f ? 1.f : q;
        out[2] = ok ? 1.f : 0.f;
        out[3] = 0.f;
        if (!ok && skipped != nullptr) *skipped += 1;
    }
}

__global__ void __launch_bounds__(256) grad_scale_kernel(const BbdmOptChunk* __restrict__ table, const float* __restrict__ clip) {
    const BbdmOptChunk c = table[blockIdx.x];
    float* __restrict__ g = const_cast<float*>(c.grad);
    if (g == nullptr) return;
    const float coef = clip[1];
    const int n = c.n;
    if (((uintptr_t)g & 15) == 0) {
        const int n4 = n >> 2;
        for (int i = threadIdx.x; i < n4; i += 256) {
            float4 v = reinterpret_cast<float4*>(g)[i];
            v.x *= coef; v.y *= coef; v.z *= coef; v.w *= coef;
            reinterpret_cast<float4*>(g)[i] = v;
        }
        for (int i = (n4 << 2) + threadIdx.x; i < n; i += 256) g[i] *= coef;
    } else {
        for (int i = threadIdx.x; i < n; i += 256) g[i] *= coef;
    }
}

}  // namespace

extern "C" int bbdm_opt_chunk_elems(void) { return CHUNK; }

static int adam_ema_launch(const BbdmOptChunk* table, int nchunks, int do_adam, double lr, double beta1, double beta2, double eps,
                           double weight_decay, long long step, int ema_mode, double ema_decay, const float* clip,
                           int skip_nonfinite, void* stream) {
    BBDM_REQUIRE(table && nchunks > 0, "adam_ema: empty chunk table");
    BBDM_REQUIRE(do_adam || ema_mode, "adam_ema: nothing to do");
    BBDM_REQUIRE(ema_mode >= 0 && ema_mode <= 2, "adam_ema: ema_mode=%d (0 none, 1 decay, 2 copy)", ema_mode);
    BBDM_REQUIRE(!do_adam || (step >= 1 && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0.),
                 "adam_ema: bad hyper-parameters (step=%lld beta1=%g beta2=%g eps=%g)", step, beta1, beta2, eps);
    OptArgs a;
    a.table = table;
    // hyper-parameters arrive as the Python doubles torch works with; every derived scalar is formed in double and
    // rounded to fp32 once, which is what a Python-number operand of an fp32 tensor op undergoes
    const double bc1 = do_adam ? 1.0 - pow(beta1, (double)step) : 1.0;
    const double bc2 = do_adam ? 1.0 - pow(beta2, (double)step) : 1.0;
    a.lr_over_bc1 = (float)(lr / bc1);
    a.sqrt_bc2 = (float)sqrt(bc2);
    a.b1c = (float)(1.0 - beta1);
    a.b2 = (float)beta2;
    a.b2c = (float)(1.0 - beta2);
    a.eps = (float)eps;
    a.wd = (float)weight_decay;
    a.ema_decay = (float)ema_decay;
    a.ema_c = (float)(1.0 - ema_decay);
    a.do_adam = do_adam;
    a.ema_mode = ema_mode;
    a.clip = clip;
    a.skip_nonfinite = skip_nonfinite;
    if (clip != nullptr)
        hipLaunchKernelGGL(adam_ema_kernel<true>, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(adam_ema_kernel<false>, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, a);
    BBDM_CHECK_LAUNCH("adam_ema");
    return BBDM_OK;
}

extern "C" int bbdm_adam_ema_step_f32(const BbdmOptChunk* table, int nchunks, int do_adam, double lr, double beta1,
                                      double beta2, double eps, double weight_decay, long long step, int ema_mode,
                                      double ema_decay, void* stream) {
    return adam_ema_launch(table, nchunks, do_adam, lr, beta1, beta2, eps, weight_decay, step, ema_mode, ema_decay, nullptr, 0, stream);
}

extern "C" int bbdm_adam_ema_step_clip_f32(const BbdmOptChunk* table, int nchunks, int do_adam, double lr, double beta1,
                                           double beta2, double eps, double weight_decay, long long step, int ema_mode,
                                           double ema_decay, const float* clip, int skip_nonfinite, void* stream) {
    BBDM_REQUIRE(clip != nullptr, "adam_ema_clip: clip (the finalize's output) is NULL");
    return adam_ema_launch(table, nchunks, do_adam, lr, beta1, beta2, eps, weight_decay, step, ema_mode, ema_decay, clip,
                           skip_nonfinite != 0, stream);
}

template <int RULE>
static void rule_ema_dispatch(const RuleArgs& a, int nchunks, void* stream) {
    const dim3 grid((unsigned)nchunks), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (a.mom != 0.f) {
        if (a.clip != nullptr) hipLaunchKernelGGL((rule_ema_kernel<RULE, true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((rule_ema_kernel<RULE, true, false>), grid, block, 0, st, a);
    } else {
        if (a.clip != nullptr) hipLaunchKernelGGL((rule_ema_kernel<RULE, false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((rule_ema_kernel<RULE, false, false>), grid, block, 0, st, a);
    }
}

// hyper-parameters arrive as Python doubles and are rounded to fp32 once, after any host arithmetic (1 - dampening, 1 - alpha), as in
// adam_ema_launch
static int rule_ema_common(RuleArgs& a, const BbdmOptChunk* table, int nchunks, double lr, double weight_decay, double momentum,
                           int ema_mode, double ema_decay, const float* clip, int skip_nonfinite, const char* what) {
    BBDM_REQUIRE(table && nchunks > 0, "%s: empty chunk table", what);
    BBDM_REQUIRE(ema_mode >= 0 && ema_mode <= 2, "%s: ema_mode=%d (0 none, 1 decay, 2 copy)", what, ema_mode);
    BBDM_REQUIRE(lr >= 0. && weight_decay >= 0. && momentum >= 0., "%s: bad hyper-parameters (lr=%g weight_decay=%g momentum=%g)", what,
                 lr, weight_decay, momentum);
    a.table = table;
    a.lr = (float)lr;
    a.wd = (float)weight_decay;
    a.mom = (float)momentum;
    a.damp_c = 1.f; a.alpha = 0.f; a.alpha_c = 1.f; a.eps = 0.f;
    a.nesterov = 0; a.first = 0;
    a.ema_decay = (float)ema_decay;
    a.ema_c = (float)(1.0 - ema_decay);
    a.ema_mode = ema_mode;
    a.clip = clip;
    a.skip_nonfinite = skip_nonfinite;
    return BBDM_OK;
}

static int sgd_ema_launch(const BbdmOptChunk* table, int nchunks, double lr, double momentum, double dampening, double weight_decay,
                          int nesterov, int first, int ema_mode, double ema_decay, const float* clip, int skip_nonfinite, void* stream) {
    RuleArgs a;
    const int rc = rule_ema_common(a, table, nchunks, lr, weight_decay, momentum, ema_mode, ema_decay, clip, skip_nonfinite, "sgd_ema");
    if (rc != BBDM_OK) return rc;
    BBDM_REQUIRE(!nesterov || (momentum > 0. && dampening == 0.), "sgd_ema: nesterov needs momentum > 0 and dampening == 0 (momentum=%g "
                 "dampening=%g)", momentum, dampening);
    a.damp_c = (float)(1.0 - dampening);
    a.nesterov = nesterov != 0;
    a.first = first != 0;
    rule_ema_dispatch<RULE_SGD>(a, nchunks, stream);
    BBDM_CHECK_LAUNCH("sgd_ema");
    return BBDM_OK;
}

static int rmsprop_ema_launch(const BbdmOptChunk* table, int nchunks, double lr, double alpha, double eps, double weight_decay,
                              double momentum, int ema_mode, double ema_decay, const float* clip, int skip_nonfinite, void* stream) {
    RuleArgs a;
    const int rc = rule_ema_common(a, table, nchunks, lr, weight_decay, momentum, ema_mode, ema_decay, clip, skip_nonfinite,
                                   "rmsprop_ema");
    if (rc != BBDM_OK) return rc;
    BBDM_REQUIRE(alpha >= 0. && eps >= 0., "rmsprop_ema: bad hyper-parameters (alpha=%g eps=%g)", alpha, eps);
    a.alpha = (float)alpha;
    a.alpha_c = (float)(1.0 - alpha);
    a.eps = (float)eps;
    rule_ema_dispatch<RULE_RMSPROP>(a, nchunks, stream);
    BBDM_CHECK_LAUNCH("rmsprop_ema");
    return BBDM_OK;
}

extern "C" int bbdm_sgd_ema_step_f32(const BbdmOptChunk* table, int nchunks, double lr, double momentum, double dampening,
                                     double weight_decay, int nesterov, int first, int ema_mode, double ema_decay, void* stream) {
    return sgd_ema_launch(table, nchunks, lr, momentum, dampening, weight_decay, nesterov, first, ema_mode, ema_decay, nullptr, 0, stream);
}

extern "C" int bbdm_sgd_ema_step_clip_f32(const BbdmOptChunk* table, int nchunks, double lr, double momentum, double dampening,
                                          double weight_decay, int nesterov, int first, int ema_mode, double ema_decay,
                                          const float* clip, int skip_nonfinite, void* stream) {
    BBDM_REQUIRE(clip != nullptr, "sgd_ema_clip: clip (the finalize's output) is NULL");
    return sgd_ema_launch(table, nchunks, lr, momentum, dampening, weight_decay, nesterov, first, ema_mode, ema_decay, clip,
                          skip_nonfinite != 0, stream);
}

extern "C" int bbdm_rmsprop_ema_step_f32(const BbdmOptChunk* table, int nchunks, double lr, double alpha, double eps,
                                         double weight_decay, double momentum, int ema_mode, double ema_decay, void* stream) {
    return rmsprop_ema_launch(table, nchunks, lr, alpha, eps, weight_decay, momentum, ema_mode, ema_decay, nullptr, 0, stream);
}

extern "C" int bbdm_rmsprop_ema_step_clip_f32(const BbdmOptChunk* table, int nchunks, double lr, double alpha, double eps,
                                              double weight_decay, double momentum, int ema_mode, double ema_decay, const float* clip,
                                              int skip_nonfinite, void* stream) {
    BBDM_REQUIRE(clip != nullptr, "rmsprop_ema_clip: clip (the finalize's output) is NULL");
    return rmsprop_ema_launch(table, nchunks, lr, alpha, eps, weight_decay, momentum, ema_mode, ema_decay, clip, skip_nonfinite != 0,
                              stream);
}

extern "C" size_t bbdm_grad_norm_cells_bytes(void) { return (size_t)NORM_CELLS * NORM_CELL_WORDS * sizeof(unsigned long long); }

extern "C" int bbdm_grad_sqnorm_f32(const BbdmOptChunk* table, int nchunks, unsigned long long* cells, void* stream) {
    BBDM_REQUIRE(table && nchunks > 0 && cells, "grad_sqnorm: empty chunk table or no cells");
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, table, cells);
    BBDM_CHECK_LAUNCH("grad_sqnorm");
    return BBDM_OK;
}

extern "C" int bbdm_grad_norm_finalize_f32(const unsigned long long* cells, double max_norm, float* out, long long* skipped,
                                           void* stream) {
    BBDM_REQUIRE(cells && out, "grad_norm_finalize: NULL cells / out");
    BBDM_REQUIRE(max_norm >= 0., "grad_norm_finalize: max_norm=%g (>= 0; +inf = no clipping)", max_norm);
    hipLaunchKernelGGL(grad_finalize_kernel, dim3(1), dim3(NORM_CELLS), 0, (hipStream_t)stream, cells, (float)max_norm, out, skipped);
    BBDM_CHECK_LAUNCH("grad_norm_finalize");
    return BBDM_OK;
}

extern "C" int bbdm_grad_scale_f32(const BbdmOptChunk* table, int nchunks, const float* clip, void* stream) {
    BBDM_REQUIRE(table && nchunks > 0 && clip, "grad_scale: empty chunk table or no clip buffer");
    hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, table, clip);
    BBDM_CHECK_LAUNCH("grad_scale");
    return BBDM_OK;
}
