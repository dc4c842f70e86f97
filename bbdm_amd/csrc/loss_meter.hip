// loss_meter.hip -- the training / validation loss by timestep, accumulated on the device (bbdm_amd/loss_meter.py).
//
// The reference logs one scalar per micro-step, the batch mean of |objective - objective_recon| at whatever t each image drew
// (BrownianBridgeModel.py:114-117), and reads it back every step (BaseRunner.py:417-436); its validation loss draws fresh t and fresh
// noise per call (BaseRunner.py:214-249).  Here the loss of every IMAGE is formed next to the scalar one and added into a table over
// buckets of t that lives on the device:
//   bbdm_loss_meter_per_image_f32   cells[N][4] += the fp64 block partials of |a - b| or (a - b)^2 of image n   (-> per_image[N])
//   bbdm_loss_meter_accumulate      meter[bucket(t_n)] += (v_n, v_n^2), counts[bucket(t_n)] += 1, v_n = fold(cells[n]) / per_sample
//   bbdm_loss_meter_read            fp64 sum[B], sumsq[B] of the table
// bbdm_bb_loss_f32 (bridge.hip) is not touched: the scalar loss keeps its bits, the meter reads a and b a second time.
// Every sum goes through the exact limb cells of stats_acc.h, and the partial a block adds is a function of the image's values alone:
// the blocks of an image, the elements of a block and the order in which a thread adds its elements depend on per_sample only -- not
// on N, on the image's place in the batch, or on which of the two load paths runs.  The table therefore has the same bits for any
// batch size, arrival order or split over ranks.  Built with -ffp-contract=off like bridge.hip.
#include "common.h"
#include "dispatch.h"
#include "elementwise.h"
#include "stats_acc.h"

namespace {

typedef unsigned long long u64;

constexpr int LM_CHUNK = 2048;           // elements of one image per workgroup: two groups of four per thread

// grid (cdiv(per_sample, LM_CHUNK) * N): block = (image, chunk).  Thread `tid` owns the groups of four elements tid and tid + 256 of
// its chunk and adds their terms in element order -- VEC: one 16-byte load per group and tensor (per_sample % 4 == 0 and 16-byte
// aligned pointers, the launcher checks), else element loads of the SAME groups with the tail cut at per_sample: the same sequence of
// additions, so the same partial.  The term is loss_partial_kernel's (bridge.hip): loss_term of elementwise.h.
template <bool VEC>
__global__ void __launch_bounds__(256) lm_per_image_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           u64* __restrict__ cells, int per_sample, int chunks, int loss_type) {
    const int n = blockIdx.x / chunks, chunk = blockIdx.x - n * chunks;
    const float* pa = a + (size_t)n * per_sample;
    const float* pb = b + (size_t)n * per_sample;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < LM_CHUNK / 1024; ++k) {
        const int e0 = chunk * LM_CHUNK + (k * 256 + (int)threadIdx.x) * 4;
        if (e0 >= per_sample) break;
        if (VEC) {
            const float4 x = *reinterpret_cast<const float4*>(pa + e0);
            const float4 y = *reinterpret_cast<const float4*>(pb + e0);
            s += loss_term(x.x, y.x, loss_type);
            s += loss_term(x.y, y.y, loss_type);
            s += loss_term(x.z, y.z, loss_type);
            s += loss_term(x.w, y.w, loss_type);
        } else {
            const int e1 = e0 + 4 < per_sample ? e0 + 4 : per_sample;
            for (int e = e0; e < e1; ++e) s += loss_term(pa[e], pb[e], loss_type);
        }
    }
    const double total = block_sum_down(s);
    if (threadIdx.x == 0) sa_add(cells + (size_t)n * SA_W, total);
}

__global__ void lm_per_image_final_kernel(const u64* __restrict__ cells, float* __restrict__ per_image, int N, double per_sample) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < N) per_image[n] = (float)(sa_load(cells + (size_t)n * SA_W) / per_sample);
}

// one thread per image.  The range check is made on the 64-bit t: 2^40 + 3 is rejected, not bucketed as 3.
__global__ void lm_accumulate_kernel(const u64* __restrict__ cells, const int64_t* __restrict__ t, u64* __restrict__ meter,
                                     u64* __restrict__ counts, int N, double per_sample, int T, int B) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int64_t tv = t[n];
    if (tv < 0 || tv >= (int64_t)T) {
        atomicAdd(counts + B, 1ull);
        return;
    }
    const int bucket = (int)((tv * (int64_t)B) / (int64_t)T);          // < 2^62: tv < T < 2^31, B < 2^31
    const double v = sa_load(cells + (size_t)n * SA_W) / per_sample;   // NaN for a cell that met a non-finite partial
    sa_add(meter + ((size_t)bucket * 2 + 0) * SA_W, v);
    sa_add(meter + ((size_t)bucket * 2 + 1) * SA_W, v * v);
    atomicAdd(counts + bucket, 1ull);
}

__global__ void lm_read_kernel(const u64* __restrict__ meter, double* __restrict__ sum, double* __restrict__ sumsq, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * B) return;
    const double v = sa_load(meter + (size_t)i * SA_W);
    if (i & 1) sumsq[i >> 1] = v;
    else sum[i >> 1] = v;
}

}  // namespace

extern "C" int bbdm_loss_meter_per_image_f32(const float* a, const float* b, unsigned long long* cells, float* per_image, int N,
                                             int per_sample, int loss_type, void* stream) {
    BBDM_REQUIRE(a && b && cells && N > 0 && per_sample > 0 && (loss_type == 0 || loss_type == 1), "loss_meter_per_image: bad args");
    BBDM_REQUIRE(per_sample <= (1 << 30), "loss_meter_per_image: per_sample=%d > 2^30", per_sample);
    const int chunks = cdiv(per_sample, LM_CHUNK);
    BBDM_REQUIRE((long long)chunks * N < (1ll << 31), "loss_meter_per_image: N=%d x %d blocks per image exceed the grid", N, chunks);
    const dim3 grid((unsigned)(chunks * N));
    dispatch([&](auto VEC) {
        hipLaunchKernelGGL(lm_per_image_kernel<VEC()>, grid, dim3(256), 0, (hipStream_t)stream, a, b, cells, per_sample, chunks, loss_type);
        return BBDM_OK;
    }, per_sample % 4 == 0 && aligned16(a) && aligned16(b));
    if (per_image)
        hipLaunchKernelGGL(lm_per_image_final_kernel, dim3(cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, cells, per_image, N,
                           (double)per_sample);
    BBDM_CHECK_LAUNCH("loss_meter_per_image");
    return BBDM_OK;
}

extern "C" int bbdm_loss_meter_accumulate(const unsigned long long* cells, const int64_t* t, unsigned long long* meter,
                                          unsigned long long* counts, int N, int per_sample, int T, int B, void* stream) {
    BBDM_REQUIRE(cells && t && meter && counts && N > 0 && per_sample > 0, "loss_meter_accumulate: bad args");
    BBDM_REQUIRE(T > 0 && B > 0, "loss_meter_accumulate: T=%d B=%d", T, B);
    hipLaunchKernelGGL(lm_accumulate_kernel, dim3(cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, cells, t, meter, counts, N,
                       (double)per_sample, T, B);
    BBDM_CHECK_LAUNCH("loss_meter_accumulate");
    return BBDM_OK;
}

extern "C" int bbdm_loss_meter_read(const unsigned long long* meter, double* sum, double* sumsq, int B, void* stream) {
    BBDM_REQUIRE(meter && sum && sumsq && B > 0 && B < (1 << 30), "loss_meter_read: bad args");
    hipLaunchKernelGGL(lm_read_kernel, dim3(cdiv(2 * B, 256)), dim3(256), 0, (hipStream_t)stream, meter, sum, sumsq, B);
    BBDM_CHECK_LAUNCH("loss_meter_read");
    return BBDM_OK;
}
