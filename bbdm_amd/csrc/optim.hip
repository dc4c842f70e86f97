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
//   rule_ema_kernel<.., CLIP = true>  g * coef (one rounding, as grads.mul_(coef)) in front of the rule; ok == 0 under skip_nonfinite: no
//                        update (the EMA part still runs, as the runner's ema.update would).
//   grad_scale_kernel    g *= coef (the standalone clip_grad_norm_).
// rule_ema_kernel is the one update kernel: Adam, and the SGD and RMSprop rules (runners/utils.py:52-55), as instances of one template
// on one walk over the chunk (chunk_walk), with the same clip buffer and EMA part.
#include "common.h"
#include "dispatch.h"
#include "stats_acc.h"

namespace {

constexpr int CHUNK = 16384;       // elements per table entry = per workgroup (64 per thread)

enum { RULE_SGD = 0, RULE_RMSPROP = 1, RULE_ADAM = 2 };

// One launch's arguments, whatever the rule (a rule reads its own fields; the launchers zero the rest).
struct OptArgs {
    const BbdmOptChunk* table;
    float lr, wd, eps;                                            // Adam: lr = lr / bc1
    float sqrt_bc2, b1c, b2, b2c;                                 // Adam: b1c = 1 - beta1, b2c = 1 - beta2
    float mom, damp_c, alpha, alpha_c;                            // SGD / RMSprop: damp_c = 1 - dampening, alpha_c = 1 - alpha
    int nesterov, first;                                          // first: SGD's first step with momentum: buf = g' (buf is not read)
    float ema_decay, ema_c;                                       // ema_c = 1 - decay
    int ema_mode;                                                 // 0 none, 1 decay, 2 copy
    const float* clip;                                            // CLIP kernels: {norm, coef, ok, 0} of grad_finalize_kernel
    int skip_nonfinite;
};

// ---- the update rules of runners/utils.py:48-57 (Adam, RMSProp, SGD) on the same chunk table (ABI 30 added the last two) --------------
// torch's single-tensor formulas (_single_tensor_adam / _sgd / _rmsprop), operation by operation.  An add with a Python-number
// alpha (grad.add(param, alpha=wd), buf.add_(grad, alpha=1 - dampening), param.add_(grad, alpha=-lr)) is ONE rounding in ATen's CPU
// kernels: fmaf here; addcmul / addcdiv are written out.
//   Adam     the header's four lines
//   SGD      g' = g + wd * p;  buf = first ? g' : momentum * buf + (1 - dampening) * g';  g' = nesterov ? g' + momentum * buf : buf;
//            p = p - lr * g'                                                  (the buf lines only with momentum != 0)
//   RMSprop  g' = g + wd * p;  sq = alpha * sq + (1 - alpha) * g' * g';  avg = sqrt(sq) + eps;
//            momentum != 0: buf = momentum * buf + g' / avg, p = p - lr * buf;  else p = p - lr * (g' / avg)
// The table's exp_avg slot carries Adam's first moment or the momentum buffer (NULL without momentum), the exp_avg_sq slot Adam's second
// moment or RMSprop's square_avg (NULL for SGD).
template <int RULE, bool MOM>
__device__ __forceinline__ void rule_one(const OptArgs& a, float& p, float g, float& buf, float& sq) {
    if (a.wd != 0.f) g = fmaf(a.wd, p, g);          // grad.add(param, alpha=wd): one rounding in ATen's kernels
    if (RULE == RULE_ADAM) {
        // at::lerp: |w| < 0.5 ? a + w (b - a) : b - (b - a) (1 - w),  w = 1 - beta1
        buf = a.b1c < 0.5f ? buf + a.b1c * (g - buf) : g - (g - buf) * (1.f - a.b1c);
        sq = sq * a.b2 + a.b2c * g * g;
        const float denom = sqrtf(sq) / a.sqrt_bc2 + a.eps;
        p = p - a.lr * (buf / denom);
    } else if (RULE == RULE_SGD) {
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

// EMA.update (runners/base/EMA.py:21-29): shadow = (1 - d) * p + d * shadow
__device__ __forceinline__ float ema_blend(const OptArgs& a, float p, float shadow) { return a.ema_c * p + a.ema_decay * shadow; }

// W consecutive floats of a chunk: one 128-bit access (W = 4, i counts groups of four) or one element (W = 1, i counts elements).
template <int W>
struct Lanes {
    float v[W];
};

template <int W>
__device__ __forceinline__ Lanes<W> load_lanes(const float* p, int i) {
    Lanes<W> r;
    if constexpr (W == 4) {
        const float4 f = reinterpret_cast<const float4*>(p)[i];
        r.v[0] = f.x, r.v[1] = f.y, r.v[2] = f.z, r.v[3] = f.w;
    } else {
        r.v[0] = p[i];
    }
    return r;
}

template <int W>
__device__ __forceinline__ void store_lanes(float* p, int i, const Lanes<W>& r) {
    if constexpr (W == 4) reinterpret_cast<float4*>(p)[i] = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else p[i] = r.v[0];
}

// The walk of one workgroup over its chunk of n elements: f(int_tag<4>, i) for thread-strided groups of four and then f(int_tag<1>, i)
// for the tail's elements when every pointer f touches is 16-byte aligned (`aligned`), else f(int_tag<1>, i) for all of the chunk.
template <class F>
__device__ __forceinline__ void chunk_walk(int n, bool aligned, F f) {
    int done = 0;
    if (aligned) {
        const int n4 = n >> 2;
        for (int i = threadIdx.x; i < n4; i += 256) f(int_tag<4>{}, i);
        done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < n; i += 256) f(int_tag<1>{}, i);
}

// One rule's update and the EMA part over one chunk per workgroup.  MOM: the rule reads / writes the exp_avg slot (Adam always),
// UPDATE = false: the EMA part alone, whatever the table holds (Adam's do_adam = 0), CLIP: g * coef (one rounding, as grads.mul_(coef))
// in front of the rule; ok == 0 under skip_nonfinite: no update (the EMA part still runs, as the runner's ema.update would).  A chunk
// whose gradient, or a state tensor the rule needs, is NULL gets no update either: a parameter without a gradient is skipped, as torch
// does.
template <int RULE, bool MOM, bool UPDATE, bool CLIP>
__global__ void __launch_bounds__(256) rule_ema_kernel(const OptArgs a) {
    constexpr bool SQ = RULE != RULE_SGD;
    const BbdmOptChunk c = a.table[blockIdx.x];
    float* __restrict__ p = c.param;
    const float* __restrict__ g = c.grad;
    float* __restrict__ m = c.exp_avg;
    float* __restrict__ v = c.exp_avg_sq;
    float* __restrict__ s = c.shadow;
    bool upd = UPDATE && g != nullptr && (!MOM || m != nullptr) && (!SQ || v != nullptr);
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
    chunk_walk(c.n, (al & 15) == 0, [&](auto W, int i) {
        constexpr int w = decltype(W)::value;
        Lanes<w> pv = load_lanes<w>(p, i);
        if (upd) {
            const Lanes<w> gv = load_lanes<w>(g, i);
            Lanes<w> mv = {}, vv = {};
            if (rd_m) mv = load_lanes<w>(m, i);
            if (SQ) vv = load_lanes<w>(v, i);
#pragma unroll
            for (int j = 0; j < w; ++j) rule_one<RULE, MOM>(a, pv.v[j], CLIP ? gv.v[j] * coef : gv.v[j], mv.v[j], vv.v[j]);
            if (MOM) store_lanes<w>(m, i, mv);
            if (SQ) store_lanes<w>(v, i, vv);
            store_lanes<w>(p, i, pv);
        }
        if (ema) {
            Lanes<w> sv = pv;
            if (a.ema_mode == 1) {
                const Lanes<w> o = load_lanes<w>(s, i);
#pragma unroll
                for (int j = 0; j < w; ++j) sv.v[j] = ema_blend(a, pv.v[j], o.v[j]);
            }
            store_lanes<w>(s, i, sv);
        }
    });
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
    chunk_walk(c.n, ((uintptr_t)g & 15) == 0, [&](auto W, int i) {
        constexpr int w = decltype(W)::value;
        Lanes<w> v = load_lanes<w>(g, i);
#pragma unroll
        for (int j = 0; j < w; ++j) v.v[j] *= coef;
        store_lanes<w>(g, i, v);
    });
}

}  // namespace

extern "C" int bbdm_opt_chunk_elems(void) { return CHUNK; }

// What every rule's launcher starts with: the shared checks and fields, every other field zero.  Hyper-parameters arrive as the Python
// doubles torch works with; every derived scalar (lr / bc1, 1 - beta, 1 - dampening, 1 - alpha, 1 - decay) is formed in double and rounded
// to fp32 once, which is what a Python-number operand of an fp32 tensor op undergoes.
static int opt_args_common(OptArgs& a, const char* what, const BbdmOptChunk* table, int nchunks, double lr, double weight_decay,
                           int ema_mode, double ema_decay, const float* clip, int skip_nonfinite) {
    BBDM_REQUIRE(table && nchunks > 0, "%s: empty chunk table", what);
    BBDM_REQUIRE(ema_mode >= 0 && ema_mode <= 2, "%s: ema_mode=%d (0 none, 1 decay, 2 copy)", what, ema_mode);
    a = OptArgs{};
    a.table = table;
    a.lr = (float)lr;
    a.wd = (float)weight_decay;
    a.ema_decay = (float)ema_decay;
    a.ema_c = (float)(1.0 - ema_decay);
    a.ema_mode = ema_mode;
    a.clip = clip;
    a.skip_nonfinite = skip_nonfinite;
    return BBDM_OK;
}

template <int RULE, bool MOM, bool UPDATE, bool CLIP>
static int rule_ema_launch(const OptArgs& a, int nchunks, void* stream, const char* what) {
    hipLaunchKernelGGL((rule_ema_kernel<RULE, MOM, UPDATE, CLIP>), dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, a);
    BBDM_CHECK_LAUNCH(what);
    return BBDM_OK;
}

static int adam_ema_launch(const BbdmOptChunk* table, int nchunks, int do_adam, double lr, double beta1, double beta2, double eps,
                           double weight_decay, long long step, int ema_mode, double ema_decay, const float* clip,
                           int skip_nonfinite, void* stream) {
    OptArgs a;
    const double bc1 = do_adam ? 1.0 - pow(beta1, (double)step) : 1.0;
    const double bc2 = do_adam ? 1.0 - pow(beta2, (double)step) : 1.0;
    if (const int rc = opt_args_common(a, "adam_ema", table, nchunks, lr / bc1, weight_decay, ema_mode, ema_decay, clip, skip_nonfinite))
        return rc;
    BBDM_REQUIRE(do_adam || ema_mode, "adam_ema: nothing to do");
    BBDM_REQUIRE(!do_adam || (step >= 1 && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0.),
                 "adam_ema: bad hyper-parameters (step=%lld beta1=%g beta2=%g eps=%g)", step, beta1, beta2, eps);
    a.sqrt_bc2 = (float)sqrt(bc2);
    a.b1c = (float)(1.0 - beta1);
    a.b2 = (float)beta2;
    a.b2c = (float)(1.0 - beta2);
    a.eps = (float)eps;
    return dispatch([&](auto UPDATE, auto CLIP) { return rule_ema_launch<RULE_ADAM, true, UPDATE(), CLIP()>(a, nchunks, stream, "adam_ema"); },
                    do_adam != 0, clip != nullptr);
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

// SGD and RMSprop: the checks and fields the two share
static int rule_ema_common(OptArgs& a, const BbdmOptChunk* table, int nchunks, double lr, double weight_decay, double momentum,
                           int ema_mode, double ema_decay, const float* clip, int skip_nonfinite, const char* what) {
    if (const int rc = opt_args_common(a, what, table, nchunks, lr, weight_decay, ema_mode, ema_decay, clip, skip_nonfinite)) return rc;
    BBDM_REQUIRE(lr >= 0. && weight_decay >= 0. && momentum >= 0., "%s: bad hyper-parameters (lr=%g weight_decay=%g momentum=%g)", what,
                 lr, weight_decay, momentum);
    a.mom = (float)momentum;
    a.damp_c = 1.f;
    a.alpha_c = 1.f;
    return BBDM_OK;
}

template <int RULE>
static int rule_ema_dispatch(const OptArgs& a, int nchunks, void* stream, const char* what) {
    return dispatch([&](auto MOM, auto CLIP) { return rule_ema_launch<RULE, MOM(), true, CLIP()>(a, nchunks, stream, what); },
                    a.mom != 0.f, a.clip != nullptr);
}

static int sgd_ema_launch(const BbdmOptChunk* table, int nchunks, double lr, double momentum, double dampening, double weight_decay,
                          int nesterov, int first, int ema_mode, double ema_decay, const float* clip, int skip_nonfinite, void* stream) {
    OptArgs a;
    const int rc = rule_ema_common(a, table, nchunks, lr, weight_decay, momentum, ema_mode, ema_decay, clip, skip_nonfinite, "sgd_ema");
    if (rc != BBDM_OK) return rc;
    BBDM_REQUIRE(!nesterov || (momentum > 0. && dampening == 0.), "sgd_ema: nesterov needs momentum > 0 and dampening == 0 (momentum=%g "
                 "dampening=%g)", momentum, dampening);
    a.damp_c = (float)(1.0 - dampening);
    a.nesterov = nesterov != 0;
    a.first = first != 0;
    return rule_ema_dispatch<RULE_SGD>(a, nchunks, stream, "sgd_ema");
}

static int rmsprop_ema_launch(const BbdmOptChunk* table, int nchunks, double lr, double alpha, double eps, double weight_decay,
                              double momentum, int ema_mode, double ema_decay, const float* clip, int skip_nonfinite, void* stream) {
    OptArgs a;
    const int rc = rule_ema_common(a, table, nchunks, lr, weight_decay, momentum, ema_mode, ema_decay, clip, skip_nonfinite,
                                   "rmsprop_ema");
    if (rc != BBDM_OK) return rc;
    BBDM_REQUIRE(alpha >= 0. && eps >= 0., "rmsprop_ema: bad hyper-parameters (alpha=%g eps=%g)", alpha, eps);
    a.alpha = (float)alpha;
    a.alpha_c = (float)(1.0 - alpha);
    a.eps = (float)eps;
    return rule_ema_dispatch<RULE_RMSPROP>(a, nchunks, stream, "rmsprop_ema");
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
