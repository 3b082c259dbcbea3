// Plain SGD with the weights-distance penalty on a flat bucket for gfx950 (reference: demo/train.py:157-186 with
// --fine_tuning, src/losses/weights_distance_loss.py): optim.FlatSGD steps through sei_sgd_fused. One HBM-bound streaming
// pass -- 18 bytes per element (p read and written, g, the anchor, the bf16 copy) plus 1/16 byte of coefficient table --
// and a one-workgroup finish that adds the per-workgroup penalty sums in a fixed order (no floating-point atomics: the
// penalty is the same bits from run to run).
// The same pass with torch.optim.Adam's update in place of SGD's (--fine_tuning --optimizer Adam): optim.FlatAdam with an
// anchor or frozen ranges steps through sei_adam_anchor_fused -- 34 bytes per element (p and both moments read and
// written, g, the anchor, the bf16 copy) plus the same 1/16 byte of table, against sei_adam_fused's 30 -- and shares the
// double wave sum and the finish kernel.
#include "sei_common.h"

namespace {

constexpr int SGD_THREADS = 256;
constexpr unsigned SGD_GRID_CAP = 1u << 20;      // one two-quad iteration per thread, as sei_adam_fused (tools/exp_sgd.py)
constexpr int FINISH_THREADS = 256;

inline unsigned sgd_grid(size_t nquads, int grid_cap) {
    return sei_capped_grid(nquads, SGD_THREADS * 2, grid_cap > 0 ? (unsigned)grid_cap : SGD_GRID_CAP);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Quads [q0, q1) of the bucket (absolute quad indices: the coefficient of quad q is coef64[q / 16], one float per 64-element
// block, which models/_flat.py never lets two parameters share). Per element, in float32 and without contraction:
//   d = p - a;  g' = gscale * g + (2 c) d;  pen += (c d) d  [from the p BEFORE the update];  p -= lr g'
// The per-thread penalty sum is kept in double (positive terms, a handful per thread), the workgroup's sum is a fixed
// shuffle tree: partials[blockIdx.x] depends on the launch shape only.
template <bool ANCHOR>
__global__ __launch_bounds__(SGD_THREADS) void sgd_vec_kernel(float *__restrict__ p, const float *__restrict__ g,
                                                              const float *__restrict__ a,
                                                              const float *__restrict__ coef64, size_t q0, size_t q1,
                                                              float lr, float gscale, unsigned short *__restrict__ p16,
                                                              double *__restrict__ partials) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    double pen = 0.0;
    auto element = [&](float pi, float gi, float ai, float c) {
        float gp = gscale * gi;
        if (ANCHOR) {
            const float d = pi - ai;
            gp = gp + (2.f * c) * d;
            pen += (double)((c * d) * d);
        }
        return pi - lr * gp;
    };
    auto update = [&](size_t q, const float4 pq, const float4 gq, const float4 aq, float c) {
        float4 o;
        o.x = element(pq.x, gq.x, aq.x, c);
        o.y = element(pq.y, gq.y, aq.y, c);
        o.z = element(pq.z, gq.z, aq.z, c);
        o.w = element(pq.w, gq.w, aq.w, c);
        reinterpret_cast<float4 *>(p)[q] = o;
        if (p16) {
            reinterpret_cast<uint2 *>(p16)[q] = make_uint2(sei_pack2_bf16(o.x, o.y), sei_pack2_bf16(o.z, o.w));
        }
    };
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    size_t q = q0 + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; q + stride < q1; q += 2 * stride) {              // two quads per stream in flight
        const size_t q2 = q + stride;
        const float4 pa = reinterpret_cast<float4 *>(p)[q], pb = reinterpret_cast<float4 *>(p)[q2];
        const float4 ga = reinterpret_cast<const float4 *>(g)[q], gb = reinterpret_cast<const float4 *>(g)[q2];
        const float4 aa = ANCHOR ? reinterpret_cast<const float4 *>(a)[q] : zero;
        const float4 ab = ANCHOR ? reinterpret_cast<const float4 *>(a)[q2] : zero;
        const float ca = ANCHOR ? coef64[q >> 4] : 0.f, cb = ANCHOR ? coef64[q2 >> 4] : 0.f;
        update(q, pa, ga, aa, ca);
        update(q2, pb, gb, ab, cb);
    }
    if (q < q1)
        update(q, reinterpret_cast<float4 *>(p)[q], reinterpret_cast<const float4 *>(g)[q],
               ANCHOR ? reinterpret_cast<const float4 *>(a)[q] : zero, ANCHOR ? coef64[q >> 4] : 0.f);
    if (ANCHOR) {
        __shared__ double scratch[SGD_THREADS / 64];
        pen = wave_sum_f64(pen);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) scratch[wave] = pen;
        __syncthreads();
        if (threadIdx.x == 0) {
            double r = scratch[0];
#pragma unroll
            for (int w = 1; w < SGD_THREADS / 64; ++w) r += scratch[w];
            partials[blockIdx.x] = r;
        }
    }
}

// torch.optim.Adam on quads [q0, q1) with the same penalty: sgd_vec_kernel's g' (same order, same double penalty sum, same
// shuffle tree, so sgd_penalty_finish_kernel folds either kernel's partials), then sei_adam_element on (p, g', m, v) --
// adam_vec_kernel's arithmetic, bit for bit, where there is no anchor or d = 0. Both moments and the bf16 copy are written
// in the same pass; nothing outside [q0, q1) is read or written.
template <bool ANCHOR>
__global__ __launch_bounds__(SGD_THREADS) void adam_anchor_vec_kernel(
    float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
    const float *__restrict__ a, const float *__restrict__ coef64, size_t q0, size_t q1, float beta1, float beta2,
    float eps, float wd, float step_size, float inv_bc2_sqrt, float gscale, unsigned short *__restrict__ p16,
    double *__restrict__ partials) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    double pen = 0.0;
    auto element = [&](float pi, float gi, float &mi, float &vi, float ai, float c) {
        float gp = gscale * gi;
        if (ANCHOR) {
            const float d = pi - ai;
            gp = gp + (2.f * c) * d;
            pen += (double)((c * d) * d);
        }
        return sei_adam_element(pi, gp, mi, vi, beta1, beta2, eps, wd, step_size, inv_bc2_sqrt);
    };
    auto update = [&](size_t q, const float4 pq, const float4 gq, float4 mq, float4 vq, const float4 aq, float c) {
        float4 o;
        o.x = element(pq.x, gq.x, mq.x, vq.x, aq.x, c);
        o.y = element(pq.y, gq.y, mq.y, vq.y, aq.y, c);
        o.z = element(pq.z, gq.z, mq.z, vq.z, aq.z, c);
        o.w = element(pq.w, gq.w, mq.w, vq.w, aq.w, c);
        reinterpret_cast<float4 *>(m)[q] = mq;
        reinterpret_cast<float4 *>(v)[q] = vq;
        reinterpret_cast<float4 *>(p)[q] = o;
        if (p16) {
            reinterpret_cast<uint2 *>(p16)[q] = make_uint2(sei_pack2_bf16(o.x, o.y), sei_pack2_bf16(o.z, o.w));
        }
    };
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    size_t q = q0 + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; q + stride < q1; q += 2 * stride) {              // two quads per stream in flight
        const size_t q2 = q + stride;
        const float4 pa = reinterpret_cast<float4 *>(p)[q], pb = reinterpret_cast<float4 *>(p)[q2];
        const float4 ma = reinterpret_cast<float4 *>(m)[q], mb = reinterpret_cast<float4 *>(m)[q2];
        const float4 va = reinterpret_cast<float4 *>(v)[q], vb = reinterpret_cast<float4 *>(v)[q2];
        const float4 ga = reinterpret_cast<const float4 *>(g)[q], gb = reinterpret_cast<const float4 *>(g)[q2];
        const float4 aa = ANCHOR ? reinterpret_cast<const float4 *>(a)[q] : zero;
        const float4 ab = ANCHOR ? reinterpret_cast<const float4 *>(a)[q2] : zero;
        const float ca = ANCHOR ? coef64[q >> 4] : 0.f, cb = ANCHOR ? coef64[q2 >> 4] : 0.f;
        update(q, pa, ga, ma, va, aa, ca);
        update(q2, pb, gb, mb, vb, ab, cb);
    }
    if (q < q1)
        update(q, reinterpret_cast<float4 *>(p)[q], reinterpret_cast<const float4 *>(g)[q],
               reinterpret_cast<float4 *>(m)[q], reinterpret_cast<float4 *>(v)[q],
               ANCHOR ? reinterpret_cast<const float4 *>(a)[q] : zero, ANCHOR ? coef64[q >> 4] : 0.f);
    if (ANCHOR) {
        __shared__ double scratch[SGD_THREADS / 64];
        pen = wave_sum_f64(pen);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) scratch[wave] = pen;
        __syncthreads();
        if (threadIdx.x == 0) {
            double r = scratch[0];
#pragma unroll
            for (int w = 1; w < SGD_THREADS / 64; ++w) r += scratch[w];
            partials[blockIdx.x] = r;
        }
    }
}

// One workgroup: thread t adds its contiguous share of the partial sums in index order, thread 0 the 256 shares in index
// order; double throughout, one float32 result.
__global__ __launch_bounds__(FINISH_THREADS) void sgd_penalty_finish_kernel(const double *__restrict__ partials,
                                                                           size_t count, float *__restrict__ out) {
    __shared__ double share[FINISH_THREADS];
    const size_t chunk = (count + FINISH_THREADS - 1) / FINISH_THREADS;
    const size_t lo = (size_t)threadIdx.x * chunk;
    const size_t hi = lo + chunk < count ? lo + chunk : count;
    double r = 0.0;
    for (size_t i = lo; i < hi; ++i) r += partials[i];
    share[threadIdx.x] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int t = 0; t < FINISH_THREADS; ++t) total += share[t];
        out[0] = (float)total;
    }
}

}  // namespace

extern "C" size_t sei_sgd_partials(size_t lo, size_t hi, int grid_cap) {
    if (hi <= lo || ((lo | hi) & 3)) return 0;
    return sgd_grid((hi - lo) / 4, grid_cap);
}

extern "C" int sei_sgd_fused(float *param, const float *grad, const float *anchor, const float *coef64, size_t lo,
                             size_t hi, float lr, float grad_scale, uint16_t *param_bf16, double *partials,
                             int grid_cap, void *stream) {
    SEI_REQUIRE(param && grad && hi > lo && grid_cap >= 0);
    SEI_REQUIRE(((lo | hi) & 3) == 0);                                      // whole quads
    SEI_REQUIRE((anchor != nullptr) == (coef64 != nullptr) && (anchor != nullptr) == (partials != nullptr));
    SEI_REQUIRE(!anchor || ((lo | hi) & 63) == 0);                          // whole blocks of the coefficient table
    SEI_REQUIRE(((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) |
                  reinterpret_cast<uintptr_t>(anchor)) & 15) == 0);
    SEI_REQUIRE((reinterpret_cast<uintptr_t>(param_bf16) & 7) == 0 && (reinterpret_cast<uintptr_t>(coef64) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(partials) & 7) == 0);
    const size_t q0 = lo / 4, q1 = hi / 4;
    const dim3 grid(sgd_grid(q1 - q0, grid_cap)), block(SGD_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (anchor)
        hipLaunchKernelGGL(sgd_vec_kernel<true>, grid, block, 0, s, param, grad, anchor, coef64, q0, q1, lr, grad_scale,
                           param_bf16, partials);
    else
        hipLaunchKernelGGL(sgd_vec_kernel<false>, grid, block, 0, s, param, grad, anchor, coef64, q0, q1, lr, grad_scale,
                           param_bf16, partials);
    return sei_launch_status();
}

extern "C" size_t sei_adam_anchor_partials(size_t lo, size_t hi, int grid_cap) {
    return sei_sgd_partials(lo, hi, grid_cap);
}

extern "C" int sei_adam_anchor_fused(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                                     const float *anchor, const float *coef64, size_t lo, size_t hi, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, int step,
                                     float grad_scale, uint16_t *param_bf16, double *partials, int grid_cap,
                                     void *stream) {
    SEI_REQUIRE(param && grad && exp_avg && exp_avg_sq && hi > lo && grid_cap >= 0 && step >= 1);
    SEI_REQUIRE(((lo | hi) & 3) == 0);                                      // whole quads
    SEI_REQUIRE((anchor != nullptr) == (coef64 != nullptr) && (anchor != nullptr) == (partials != nullptr));
    SEI_REQUIRE(!anchor || ((lo | hi) & 63) == 0);                          // whole blocks of the coefficient table
    SEI_REQUIRE(((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) |
                  reinterpret_cast<uintptr_t>(exp_avg) | reinterpret_cast<uintptr_t>(exp_avg_sq) |
                  reinterpret_cast<uintptr_t>(anchor)) & 15) == 0);
    SEI_REQUIRE((reinterpret_cast<uintptr_t>(param_bf16) & 7) == 0 && (reinterpret_cast<uintptr_t>(coef64) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(partials) & 7) == 0);
    // the two scalars exactly as sei_adam_fused derives them: double pow and sqrt, rounded once
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    const float step_size = (float)((double)lr / bc1);
    const float inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    const size_t q0 = lo / 4, q1 = hi / 4;
    const dim3 grid(sgd_grid(q1 - q0, grid_cap)), block(SGD_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (anchor)
        hipLaunchKernelGGL(adam_anchor_vec_kernel<true>, grid, block, 0, s, param, grad, exp_avg, exp_avg_sq, anchor,
                           coef64, q0, q1, beta1, beta2, eps, weight_decay, step_size, inv_bc2_sqrt, grad_scale,
                           param_bf16, partials);
    else
        hipLaunchKernelGGL(adam_anchor_vec_kernel<false>, grid, block, 0, s, param, grad, exp_avg, exp_avg_sq, anchor,
                           coef64, q0, q1, beta1, beta2, eps, weight_decay, step_size, inv_bc2_sqrt, grad_scale,
                           param_bf16, partials);
    return sei_launch_status();
}

extern "C" int sei_sgd_penalty_finish(const double *partials, size_t count, float *penalty, void *stream) {
    SEI_REQUIRE(partials && penalty && count > 0);
    SEI_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7) == 0 && (reinterpret_cast<uintptr_t>(penalty) & 3) == 0);
    hipLaunchKernelGGL(sgd_penalty_finish_kernel, dim3(1), dim3(FINISH_THREADS), 0, (hipStream_t)stream, partials, count,
                       penalty);
    return sei_launch_status();
}
