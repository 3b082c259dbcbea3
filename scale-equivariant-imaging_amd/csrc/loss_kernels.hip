// Loss-side streaming kernels for gfx950: axpy (noise / SURE probe), fused SURE terms + gradients,
// fused MSE + gradient. HBM-bound; reductions are two-stage (per-block partials in a caller-provided
// workspace, then one finishing block) so results are bitwise reproducible run to run (no float atomics).
//
//   sei_axpy       : y + sigma*n (deepinv GaussianNoise), y + tau*b (losses/sure.py:24)
//   sei_sure_terms : losses/sure.py:24-31 (mc_div) and :57-62 (cropped mse) + d/dy1, d/dy2
//   sei_mse_terms  : deepinv `mse` metric inside EILoss (losses/__init__.py:117-122) + d/dx3
//   sei_sure_loss_unsure : losses/sure.py:24-31,57-66 with sigma^2 replaced by a device-resident multiplier and its ascent
//                    step (UNSURE, Tachella, Davies, Jacques; restated from the paper, no reference lines: the reference's
//                    sure.py predates it)
//   sei_axpy_sqrt_dev : y + sqrt(max(eta, 0))*n, deepinv GaussianNoise with the multiplier read from device memory
//   sei_sure_loss_unsure_pg : the same for Poisson-Gaussian noise (variance sigma^2 + gain * signal) with both levels unknown:
//                    the weight in front of the divergence is eta + gamma y per pixel, two multipliers with one ascent step
//                    each (Poisson-Gaussian UNSURE, the same paper; restated from it, no reference lines)
//   sei_axpy_hetero_dev : y + sqrt(max(eta + gamma y, 0))*n, the noise of that model at the two multipliers in device memory
#include <cmath>

#include "sei_common.h"

namespace {

constexpr int RED_THREADS = 256;

// out = a + alpha(a) b. The factor of b: one value for the whole launch (ConstAlpha), or the Poisson-Gaussian standard
// deviation at the signal a, sqrt(max(eta + gamma a, 0)) (HeteroAlpha).
struct ConstAlpha {
    float alpha;
    __device__ __forceinline__ float operator()(float) const { return alpha; }
};
struct HeteroAlpha {
    float eta, gamma;
    __device__ __forceinline__ float operator()(float a) const { return sqrtf(fmaxf(fmaf(gamma, a, eta), 0.f)); }
};

template <class Alpha>
__device__ __forceinline__ void axpy_body(const float *__restrict__ a, const float *__restrict__ b, Alpha alpha,
                                          float *__restrict__ out, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t n4 = n / 4;
    const float4 *a4 = reinterpret_cast<const float4 *>(a);
    const float4 *b4 = reinterpret_cast<const float4 *>(b);
    float4 *o4 = reinterpret_cast<float4 *>(out);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 va = a4[i], vb = b4[i];
        o4[i] = make_float4(fmaf(alpha(va.x), vb.x, va.x), fmaf(alpha(va.y), vb.y, va.y), fmaf(alpha(va.z), vb.z, va.z),
                            fmaf(alpha(va.w), vb.w, va.w));
    }
    for (size_t i = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float va = a[i];
        out[i] = fmaf(alpha(va), b[i], va);
    }
}

__global__ __launch_bounds__(256) void axpy_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                   float alpha, float *__restrict__ out, size_t n) {
    axpy_body(a, b, ConstAlpha{alpha}, out, n);
}

// alpha = sqrt(max(*p, 0)) read from device memory by every thread (one cached scalar load): the UNSURE noise level
__global__ __launch_bounds__(256) void axpy_sqrt_dev_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                            const float *__restrict__ p, float *__restrict__ out,
                                                            size_t n) {
    axpy_body(a, b, ConstAlpha{sqrtf(fmaxf(*p, 0.f))}, out, n);
}

// alpha_i = sqrt(max(state[0] + state[4] a_i, 0)): the Poisson-Gaussian UNSURE state {eta, m_eta, k, 0, gamma, m_gamma, 0, 0}
__global__ __launch_bounds__(256) void axpy_hetero_dev_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                              const float *__restrict__ state, float *__restrict__ out,
                                                              size_t n) {
    axpy_body(a, b, HeteroAlpha{state[0], state[4]}, out, n);
}

// The coefficient of the divergence term at one pixel, 2 (noise variance) / n_div: one value for all pixels (ConstWeight:
// a known sigma^2, or the UNSURE multiplier), or affine in the measurement (AffineWeight: Poisson-Gaussian UNSURE,
// variance eta + gamma y; it also asks for the third sum, of y times the divergence terms). With gamma == 0 AffineWeight
// performs ConstWeight's operations on c_div = (2 eta) inv_n_div: the same bits.
struct ConstWeight {
    static constexpr bool kSignal = false;
    float c_div;
    __device__ __forceinline__ float operator()(float) const { return c_div; }
};
struct AffineWeight {
    static constexpr bool kSignal = true;
    float eta, gamma, inv_n_div;
    __device__ __forceinline__ float operator()(float yy) const { return (2.f * fmaf(gamma, yy, eta)) * inv_n_div; }
};

// stage 1: per-block partial sums of the two SURE terms (three with a signal-dependent weight: the partials then lie in the
// order div, y-weighted div, mse) + elementwise gradients
template <class Weight>
__device__ __forceinline__ void sure_terms_body(
    const float *__restrict__ y, const float *__restrict__ y1, const float *__restrict__ y2,
    const float *__restrict__ b, size_t total, int H, int W, int md, int mm, float inv_tau, float c_mse,
    Weight weight, float *__restrict__ g1, float *__restrict__ g2, float *__restrict__ work, float *scratch) {
    float s_div = 0.f, s_mse = 0.f, s_ydiv = 0.f;
    const size_t stride = (size_t)gridDim.x * RED_THREADS;
    for (size_t i = (size_t)blockIdx.x * RED_THREADS + threadIdx.x; i < total; i += stride) {
        const int p = (int)(i % ((size_t)H * W));
        const int r = p / W, c = p - r * W;
        const bool in_d = r >= md && r < H - md && c >= md && c < W - md;
        const bool in_m = r >= mm && r < H - mm && c >= mm && c < W - mm;
        const float v1 = y1[i];
        float ga = 0.f, gb = 0.f;
        if (in_d) {
            const float bb = b[i];
            const float term = bb * (y2[i] - v1) * inv_tau;
            s_div += term;
            float c_div;
            if constexpr (Weight::kSignal) {
                const float yy = y[i];
                s_ydiv += yy * term;
                c_div = weight(yy);
            } else {
                c_div = weight(0.f);
            }
            gb = c_div * bb * inv_tau;
            ga = -gb;
        }
        if (in_m) {
            const float d = v1 - y[i];
            s_mse = fmaf(d, d, s_mse);
            ga = fmaf(2.f * c_mse, d, ga);
        }
        g1[i] = ga;
        g2[i] = gb;
    }
    const float bd = sei_block_sum<RED_THREADS>(s_div, scratch);
    const float bm = sei_block_sum<RED_THREADS>(s_mse, scratch);
    if constexpr (Weight::kSignal) {
        const float by = sei_block_sum<RED_THREADS>(s_ydiv, scratch);
        if (threadIdx.x == 0) {
            work[blockIdx.x] = bd;
            work[SEI_REDUCE_BLOCKS + blockIdx.x] = by;
            work[2 * SEI_REDUCE_BLOCKS + blockIdx.x] = bm;
        }
    } else if (threadIdx.x == 0) {
        work[blockIdx.x] = bd;
        work[SEI_REDUCE_BLOCKS + blockIdx.x] = bm;
    }
}

__global__ __launch_bounds__(RED_THREADS) void sure_terms_kernel(
    const float *__restrict__ y, const float *__restrict__ y1, const float *__restrict__ y2,
    const float *__restrict__ b, size_t total, int H, int W, int md, int mm, float inv_tau, float c_mse,
    float c_div, float *__restrict__ g1, float *__restrict__ g2, float *__restrict__ work) {
    __shared__ float scratch[RED_THREADS / 64];
    sure_terms_body(y, y1, y2, b, total, H, W, md, mm, inv_tau, c_mse, ConstWeight{c_div}, g1, g2, work, scratch);
}

// stage 1 with c_div = 2 eta / n_div formed from the multiplier in device memory (state[0]; UNSURE): every workgroup reads
// it before the finishing block of the same call may move it, so the gradients carry the multiplier as it stood
__global__ __launch_bounds__(RED_THREADS) void sure_terms_unsure_kernel(
    const float *__restrict__ y, const float *__restrict__ y1, const float *__restrict__ y2,
    const float *__restrict__ b, size_t total, int H, int W, int md, int mm, float inv_tau, float c_mse,
    float inv_n_div, const float *__restrict__ state, float *__restrict__ g1, float *__restrict__ g2,
    float *__restrict__ work) {
    __shared__ float scratch[RED_THREADS / 64];
    const float c_div = (2.f * state[0]) * inv_n_div;
    sure_terms_body(y, y1, y2, b, total, H, W, md, mm, inv_tau, c_mse, ConstWeight{c_div}, g1, g2, work, scratch);
}

// stage 1 with the per-pixel weight eta + gamma y formed from the two multipliers in device memory (state[0], state[4];
// Poisson-Gaussian UNSURE), read by every workgroup before the finishing block of the same call may move them
__global__ __launch_bounds__(RED_THREADS) void sure_terms_unsure_pg_kernel(
    const float *__restrict__ y, const float *__restrict__ y1, const float *__restrict__ y2,
    const float *__restrict__ b, size_t total, int H, int W, int md, int mm, float inv_tau, float c_mse,
    float inv_n_div, const float *__restrict__ state, float *__restrict__ g1, float *__restrict__ g2,
    float *__restrict__ work) {
    __shared__ float scratch[RED_THREADS / 64];
    sure_terms_body(y, y1, y2, b, total, H, W, md, mm, inv_tau, c_mse, AffineWeight{state[0], state[4], inv_n_div}, g1, g2,
                    work, scratch);
}

__global__ __launch_bounds__(RED_THREADS) void mse_terms_kernel(const float *__restrict__ a,
                                                                const float *__restrict__ b, size_t n,
                                                                float scale, float *__restrict__ ga,
                                                                float *__restrict__ work) {
    __shared__ float scratch[RED_THREADS / 64];
    float s = 0.f;
    const size_t stride = (size_t)gridDim.x * RED_THREADS;
    for (size_t i = (size_t)blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += stride) {
        const float d = a[i] - b[i];
        s = fmaf(d, d, s);
        ga[i] = scale * d;
    }
    const float bs = sei_block_sum<RED_THREADS>(s, scratch);
    if (threadIdx.x == 0) work[blockIdx.x] = bs;
}

// sum over pixels of (Y(a) - Y(b))^2 for planar RGB images (3, npix): the numerator of the luma PSNR
__global__ __launch_bounds__(RED_THREADS) void luma_sqerr_kernel(const float *__restrict__ a,
                                                                 const float *__restrict__ b, size_t npix,
                                                                 float *__restrict__ work) {
    __shared__ float scratch[RED_THREADS / 64];
    float s = 0.f;
    const size_t stride = (size_t)gridDim.x * RED_THREADS;
    for (size_t i = (size_t)blockIdx.x * RED_THREADS + threadIdx.x; i < npix; i += stride) {
        const float ya = 0.299f * a[i] + 0.587f * a[npix + i] + 0.114f * a[2 * npix + i];
        const float yb = 0.299f * b[i] + 0.587f * b[npix + i] + 0.114f * b[2 * npix + i];
        const float d = ya - yb;
        s = fmaf(d, d, s);
    }
    const float bs = sei_block_sum<RED_THREADS>(s, scratch);
    if (threadIdx.x == 0) work[blockIdx.x] = bs;
}

// stage 2: one block sums `nparts` partials of each of `nout` quantities (stored SEI_REDUCE_BLOCKS apart)
__global__ __launch_bounds__(RED_THREADS) void finish_sums_kernel(const float *__restrict__ work, int nparts,
                                                                  int nout, float *__restrict__ out) {
    __shared__ float scratch[RED_THREADS / 64];
    for (int q = 0; q < nout; ++q) {
        float v = 0.f;
        for (int i = threadIdx.x; i < nparts; i += RED_THREADS) v += work[q * SEI_REDUCE_BLOCKS + i];
        const float s = sei_block_sum<RED_THREADS>(v, scratch);
        if (threadIdx.x == 0) out[q] = s;
    }
}

// stage 2 with the loss value formed on the device: out[nout] = sum_q coef[q] * out[q] + bias (the SURE loss = c_mse * mse sum
// + c_div * div sum - constant; the weighted mean squared error): the step's scalar arithmetic is not a chain of 0-dim
// torch kernels (round 5: five fewer launches in the forward pass of a proposed-loss step)
struct FinishCoef {
    float coef[2], bias;
};
__global__ __launch_bounds__(RED_THREADS) void finish_loss_kernel(const float *__restrict__ work, int nparts, int nout,
                                                                  FinishCoef fc, float *__restrict__ out) {
    __shared__ float scratch[RED_THREADS / 64];
    float total = fc.bias;
    for (int q = 0; q < nout; ++q) {
        float v = 0.f;
        for (int i = threadIdx.x; i < nparts; i += RED_THREADS) v += work[q * SEI_REDUCE_BLOCKS + i];
        const float s = sei_block_sum<RED_THREADS>(v, scratch);
        if (threadIdx.x == 0) out[q] = s;
        total = fmaf(fc.coef[q], s, total);             // (only thread 0's `s` is the block sum; only it writes below)
    }
    if (threadIdx.x == 0) out[nout] = total;
}

// stage 2 of the UNSURE loss: the two sums folded as finish_loss_kernel folds them, loss = c_mse mse + 2 eta d with
// d = div / n_div and eta = state[0] (no constant term), then -- `update` -- one step of gradient ASCENT on the multiplier
// along the averaged direction: g = 2 d, m' = g on the first call (k == 0) else mu m + (1 - mu) g, eta' = eta + alpha m',
// k' = k + 1. state = {eta, m, k, unused}; thread 0 alone reads and writes it, with ordinary stores.
struct UnsureStep {
    float c_mse, inv_n_div, step_size, momentum;
    int update;
};
__global__ __launch_bounds__(RED_THREADS) void finish_unsure_kernel(const float *__restrict__ work, int nparts, UnsureStep u,
                                                                    float *__restrict__ state, float *__restrict__ out) {
    __shared__ float scratch[RED_THREADS / 64];
    float sums[2];
    for (int q = 0; q < 2; ++q) {
        float v = 0.f;
        for (int i = threadIdx.x; i < nparts; i += RED_THREADS) v += work[q * SEI_REDUCE_BLOCKS + i];
        sums[q] = sei_block_sum<RED_THREADS>(v, scratch);    // (only thread 0's value is the block sum; only it goes on)
    }
    if (threadIdx.x != 0) return;
    const float eta = state[0], m = state[1], k = state[2];
    const float d = sums[0] * u.inv_n_div;
    out[0] = sums[0];
    out[1] = sums[1];
    out[2] = fmaf(u.c_mse, sums[1], (2.f * eta) * d);
    if (u.update) {
        const float g = 2.f * d;
        const float m_new = k == 0.f ? g : fmaf(u.momentum, m, (1.f - u.momentum) * g);
        state[0] = fmaf(u.step_size, m_new, eta);
        state[1] = m_new;
        state[2] = k + 1.f;
    }
}

// stage 2 of the Poisson-Gaussian UNSURE loss: three sums (div D0, y-weighted div D1, mse), loss = c_mse mse + 2 (eta d0 +
// gamma d1) with d = D / n_div, then -- `update` -- finish_unsure_kernel's ascent step for each multiplier on its own
// constraint (g = 2 d0 moves eta by step_eta, g = 2 d1 moves gamma by step_gamma; one momentum, one counter k).
// state = {eta, m_eta, k, 0, gamma, m_gamma, 0, 0}; thread 0 alone reads and writes it, with ordinary stores. With gamma == 0
// and step_gamma == 0 the loss and state[0..2] are finish_unsure_kernel's bits (a finite D1 enters as + 0).
struct UnsurePgStep {
    float c_mse, inv_n_div, step_eta, step_gamma, momentum;
    int update;
};
__global__ __launch_bounds__(RED_THREADS) void finish_unsure_pg_kernel(const float *__restrict__ work, int nparts,
                                                                       UnsurePgStep u, float *__restrict__ state,
                                                                       float *__restrict__ out) {
    __shared__ float scratch[RED_THREADS / 64];
    float sums[3];
    for (int q = 0; q < 3; ++q) {
        float v = 0.f;
        for (int i = threadIdx.x; i < nparts; i += RED_THREADS) v += work[q * SEI_REDUCE_BLOCKS + i];
        sums[q] = sei_block_sum<RED_THREADS>(v, scratch);    // (only thread 0's value is the block sum; only it goes on)
    }
    if (threadIdx.x != 0) return;
    const float eta = state[0], m_eta = state[1], k = state[2], gamma = state[4], m_gamma = state[5];
    const float d0 = sums[0] * u.inv_n_div, d1 = sums[1] * u.inv_n_div;
    out[0] = sums[0];
    out[1] = sums[1];
    out[2] = sums[2];
    out[3] = fmaf(u.c_mse, sums[2], fmaf(2.f * gamma, d1, (2.f * eta) * d0));
    if (u.update) {
        const float g0 = 2.f * d0, g1 = 2.f * d1, keep = 1.f - u.momentum;
        const float m0 = k == 0.f ? g0 : fmaf(u.momentum, m_eta, keep * g0);
        const float m1 = k == 0.f ? g1 : fmaf(u.momentum, m_gamma, keep * g1);
        state[0] = fmaf(u.step_eta, m0, eta);
        state[1] = m0;
        state[2] = k + 1.f;
        state[4] = fmaf(u.step_gamma, m1, gamma);
        state[5] = m1;
    }
}

inline int reduce_blocks(size_t n) {
    size_t g = sei_ceil_div(n, (size_t)RED_THREADS * 4);
    if (g < 1) g = 1;
    if (g > SEI_REDUCE_BLOCKS) g = SEI_REDUCE_BLOCKS;
    return (int)g;
}

// zero up to 8 slices of one buffer in one launch (the gaps of the gradient bucket between the stored weight gradients)
struct ZeroRanges {
    unsigned long long off[8], len[8], start[9];     // start: prefix sums of the lengths (in elements)
    int count;
};
__global__ __launch_bounds__(256) void zero_ranges_kernel(float *__restrict__ base, ZeroRanges r) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < r.start[r.count]; i += stride) {
        int k = 0;
        while (k + 1 < r.count && i >= r.start[k + 1]) ++k;
        base[r.off[k] + (i - r.start[k])] = 0.f;
    }
}
}  // namespace

extern "C" int sei_zero_ranges(float *base, const unsigned long long *off_len_pairs, int count, void *stream) {
    SEI_REQUIRE(base && off_len_pairs && count > 0 && count <= 8);
    ZeroRanges r;
    r.count = count;
    r.start[0] = 0;
    for (int k = 0; k < count; ++k) {
        r.off[k] = off_len_pairs[2 * k];
        r.len[k] = off_len_pairs[2 * k + 1];
        r.start[k + 1] = r.start[k] + r.len[k];
    }
    if (r.start[count] == 0) return 0;
    size_t grid = sei_ceil_div((size_t)r.start[count], 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(zero_ranges_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, base, r);
    return sei_launch_status();
}

extern "C" int sei_axpy(const float *a, const float *b, float alpha, float *out, size_t n, void *stream) {
    SEI_REQUIRE(a && b && out && n > 0);
    SEI_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15) == 0);
    size_t grid = sei_ceil_div(n / 4 + 1, 256);
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(axpy_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a, b, alpha, out, n);
    return sei_launch_status();
}

extern "C" int sei_axpy_sqrt_dev(const float *a, const float *b, const float *p, float *out, size_t n, void *stream) {
    SEI_REQUIRE(a && b && p && out && n > 0);
    SEI_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15) == 0 && ((uintptr_t)p & 3) == 0);
    size_t grid = sei_ceil_div(n / 4 + 1, 256);
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(axpy_sqrt_dev_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a, b, p, out, n);
    return sei_launch_status();
}

extern "C" int sei_axpy_hetero_dev(const float *a, const float *b, const float *state, float *out, size_t n, void *stream) {
    SEI_REQUIRE(a && b && state && out && n > 0);
    SEI_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15) == 0 && ((uintptr_t)state & 3) == 0);
    size_t grid = sei_ceil_div(n / 4 + 1, 256);
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(axpy_hetero_dev_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a, b, state, out, n);
    return sei_launch_status();
}

// The arithmetic behind the scale transform's two uniform draws (reference src/transforms.py:5-24): rate = table[floor(n u)],
// centre = 2 u' - 1 -- the float32 operations torch performs one elementwise kernel at a time, in one launch.
__global__ __launch_bounds__(256) void scale_params_kernel(const float *__restrict__ u, const float *__restrict__ v,
                                                           const float *__restrict__ table, int ntable, int B,
                                                           float *__restrict__ rate, float *__restrict__ center) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) {
        int k = (int)floorf((float)ntable * u[i]);
        k = k < 0 ? 0 : (k >= ntable ? ntable - 1 : k);            // (rand() < 1: never clamps)
        rate[i] = table[k];
    }
    if (i < 2 * B) center[i] = 2.0f * v[i] - 1.0f;
}

extern "C" int sei_scale_params(const float *u, const float *v, const float *table, int ntable, int B, float *rate,
                                float *center, void *stream) {
    SEI_REQUIRE(u && v && table && rate && center && ntable > 0 && B > 0);
    hipLaunchKernelGGL(scale_params_kernel, dim3((unsigned)sei_ceil_div((size_t)2 * B, 256)), dim3(256), 0,
                       (hipStream_t)stream, u, v, table, ntable, B, rate, center);
    return sei_launch_status();
}

extern "C" int sei_sure_terms(const float *y, const float *y1, const float *y2, const float *b, int planes,
                              int H, int W, int margin_div, int margin_mse, float tau, float c_mse,
                              float c_div, float *out2, float *g1, float *g2, float *work, void *stream) {
    SEI_REQUIRE(y && y1 && y2 && b && out2 && g1 && g2 && work);
    SEI_REQUIRE(planes > 0 && H > 0 && W > 0 && margin_div >= 0 && margin_mse >= 0 && tau != 0.f);
    SEI_REQUIRE(2 * margin_div < H && 2 * margin_div < W && 2 * margin_mse < H && 2 * margin_mse < W);
    const size_t total = (size_t)planes * H * W;
    const int grid = reduce_blocks(total);
    hipLaunchKernelGGL(sure_terms_kernel, dim3(grid), dim3(RED_THREADS), 0, (hipStream_t)stream, y, y1, y2, b,
                       total, H, W, margin_div, margin_mse, 1.0f / tau, c_mse, c_div, g1, g2, work);
    hipLaunchKernelGGL(finish_sums_kernel, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream,
                       (const float *)work, grid, 2, out2);
    return sei_launch_status();
}

// sei_sure_terms + the loss value: out3[0] = div sum, out3[1] = mse sum, out3[2] = c_mse out3[1] + c_div out3[0] - cst.
extern "C" int sei_sure_loss(const float *y, const float *y1, const float *y2, const float *b, int planes, int H, int W,
                             int margin_div, int margin_mse, float tau, float c_mse, float c_div, float cst, float *out3,
                             float *g1, float *g2, float *work, void *stream) {
    SEI_REQUIRE(y && y1 && y2 && b && out3 && g1 && g2 && work);
    SEI_REQUIRE(planes > 0 && H > 0 && W > 0 && margin_div >= 0 && margin_mse >= 0 && tau != 0.f);
    SEI_REQUIRE(2 * margin_div < H && 2 * margin_div < W && 2 * margin_mse < H && 2 * margin_mse < W);
    const size_t total = (size_t)planes * H * W;
    const int grid = reduce_blocks(total);
    hipLaunchKernelGGL(sure_terms_kernel, dim3(grid), dim3(RED_THREADS), 0, (hipStream_t)stream, y, y1, y2, b,
                       total, H, W, margin_div, margin_mse, 1.0f / tau, c_mse, c_div, g1, g2, work);
    FinishCoef fc;
    fc.coef[0] = c_div; fc.coef[1] = c_mse; fc.bias = -cst;
    hipLaunchKernelGGL(finish_loss_kernel, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream, (const float *)work, grid, 2,
                       fc, out3);
    return sei_launch_status();
}

// sei_sure_loss with the multiplier eta = state[0] in device memory in the place of sigma^2, and its ascent step (UNSURE).
extern "C" int sei_sure_loss_unsure(const float *y, const float *y1, const float *y2, const float *b, int planes, int H,
                                    int W, int margin_div, int margin_mse, float tau, float c_mse, float inv_n_div,
                                    float step_size, float momentum, int update, float *state, float *out3, float *g1,
                                    float *g2, float *work, void *stream) {
    SEI_REQUIRE(y && y1 && y2 && b && out3 && g1 && g2 && work);
    SEI_REQUIRE(planes > 0 && H > 0 && W > 0 && margin_div >= 0 && margin_mse >= 0 && tau != 0.f);
    SEI_REQUIRE(2 * margin_div < H && 2 * margin_div < W && 2 * margin_mse < H && 2 * margin_mse < W);
    SEI_REQUIRE(state && ((uintptr_t)state & 15) == 0);
    SEI_REQUIRE(momentum >= 0.f && momentum < 1.f && std::isfinite(step_size) && (update == 0 || update == 1));
    const size_t total = (size_t)planes * H * W;
    const int grid = reduce_blocks(total);
    hipLaunchKernelGGL(sure_terms_unsure_kernel, dim3(grid), dim3(RED_THREADS), 0, (hipStream_t)stream, y, y1, y2, b,
                       total, H, W, margin_div, margin_mse, 1.0f / tau, c_mse, inv_n_div, (const float *)state, g1, g2, work);
    UnsureStep u;
    u.c_mse = c_mse; u.inv_n_div = inv_n_div; u.step_size = step_size; u.momentum = momentum; u.update = update;
    hipLaunchKernelGGL(finish_unsure_kernel, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream, (const float *)work, grid,
                       u, state, out3);
    return sei_launch_status();
}

// sei_sure_loss_unsure with the per-pixel weight eta + gamma y (state[0], state[4]) and one ascent step per multiplier
// (Poisson-Gaussian UNSURE). work: 3 * SEI_REDUCE_BLOCKS floats.
extern "C" int sei_sure_loss_unsure_pg(const float *y, const float *y1, const float *y2, const float *b, int planes, int H,
                                       int W, int margin_div, int margin_mse, float tau, float c_mse, float inv_n_div,
                                       float step_eta, float step_gamma, float momentum, int update, float *state,
                                       float *out4, float *g1, float *g2, float *work, void *stream) {
    SEI_REQUIRE(y && y1 && y2 && b && out4 && g1 && g2 && work);
    SEI_REQUIRE(planes > 0 && H > 0 && W > 0 && margin_div >= 0 && margin_mse >= 0 && tau != 0.f);
    SEI_REQUIRE(2 * margin_div < H && 2 * margin_div < W && 2 * margin_mse < H && 2 * margin_mse < W);
    SEI_REQUIRE(state && ((uintptr_t)state & 15) == 0);
    SEI_REQUIRE(momentum >= 0.f && momentum < 1.f && std::isfinite(step_eta) && std::isfinite(step_gamma) &&
                (update == 0 || update == 1));
    const size_t total = (size_t)planes * H * W;
    const int grid = reduce_blocks(total);
    hipLaunchKernelGGL(sure_terms_unsure_pg_kernel, dim3(grid), dim3(RED_THREADS), 0, (hipStream_t)stream, y, y1, y2, b,
                       total, H, W, margin_div, margin_mse, 1.0f / tau, c_mse, inv_n_div, (const float *)state, g1, g2, work);
    UnsurePgStep u;
    u.c_mse = c_mse; u.inv_n_div = inv_n_div; u.step_eta = step_eta; u.step_gamma = step_gamma; u.momentum = momentum;
    u.update = update;
    hipLaunchKernelGGL(finish_unsure_pg_kernel, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream, (const float *)work,
                       grid, u, state, out4);
    return sei_launch_status();
}

// sei_mse_terms + the loss value: out2[0] = sum (a - b)^2, out2[1] = value_scale * out2[0].
extern "C" int sei_mse_loss(const float *a, const float *b, size_t n, float grad_scale, float value_scale, float *out2,
                            float *ga, float *work, void *stream) {
    SEI_REQUIRE(a && b && out2 && ga && work && n > 0);
    const int grid = reduce_blocks(n);
    hipLaunchKernelGGL(mse_terms_kernel, dim3(grid), dim3(RED_THREADS), 0, (hipStream_t)stream, a, b, n, grad_scale, ga,
                       work);
    FinishCoef fc;
    fc.coef[0] = value_scale; fc.coef[1] = 0.f; fc.bias = 0.f;
    hipLaunchKernelGGL(finish_loss_kernel, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream, (const float *)work, grid, 1,
                       fc, out2);
    return sei_launch_status();
}

extern "C" int sei_mse_terms(const float *a, const float *b, size_t n, float scale, float *out1, float *ga,
                             float *work, void *stream) {
    SEI_REQUIRE(a && b && out1 && ga && work && n > 0);
    const int grid = reduce_blocks(n);
    hipLaunchKernelGGL(mse_terms_kernel, dim3(grid), dim3(RED_THREADS), 0, (hipStream_t)stream, a, b, n, scale,
                       ga, work);
    hipLaunchKernelGGL(finish_sums_kernel, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream,
                       (const float *)work, grid, 1, out1);
    return sei_launch_status();
}


extern "C" int sei_luma_sqerr(const float *a, const float *b, size_t npix, float *out1, float *work, void *stream) {
    SEI_REQUIRE(a && b && out1 && work && npix > 0);
    const int grid = reduce_blocks(npix);
    hipLaunchKernelGGL(luma_sqerr_kernel, dim3(grid), dim3(RED_THREADS), 0, (hipStream_t)stream, a, b, npix, work);
    hipLaunchKernelGGL(finish_sums_kernel, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream,
                       (const float *)work, grid, 1, out1);
    return sei_launch_status();
}
