// The step of the DPS baseline for gfx950, float32 (models/dps.py; deepinv v0.2.0's sampling.DPS restated). Between the
// denoiser's taped forward and its vector-Jacobian product (models/drunet.py) a step launches, with every scalar on the
// device and no host read:
//
//   sei_dps_u        : u = clamp(2 out - 1, -1, 1) / 2 + 0.5, what the physics' A is applied to.
//   sei_dps_residual : r = Au - y; per image f_b = 0.5 ||r_b||^2 and s_b = 1 / (2 sqrt(f_b)) (0 where f_b = 0), written by
//                      the fold behind the reduction.
//   sei_dps_seed     : seed = A^T r where -1 <= 2 out - 1 <= 1, else 0: what the denoiser's VJP is handed.
//   sei_dps_step     : x0 = clamp(2 out - 1, -1, 1); x = ((c0 x0 + st nz) + c1 x) - (ginv s_b) gx in place;
//                      xin = x / den + 0.5, the next denoiser input (den = 2: the result of the last pair).
//
// s_b is a per-image scalar and everything between the residual and the gradient is linear, so it is applied at the end.
//
// The kernels stream B images of m >= 1 floats each from 16-byte aligned tensors: 16-byte lanes over the m / 4 quads of an
// image (grid stride over blockIdx.x, blockIdx.y the image), the m % 4 elements behind the last quad by the first lanes of
// the image's workgroup 0. Image b starts at element b m, which is 16-byte aligned whenever m % 4 == 0 (every image whose
// extents the denoiser takes); where it is not, the image's quads are the same four elements moved by four 4-byte
// accesses, so a thread's elements and the order of its sum do not depend on where the image sits. The reduction leaves
// one partial per workgroup, part[g * B + b] (a fixed shuffle tree over per-thread sums taken in index order), and one
// workgroup folds them in the order of every fold of this library (fold_entries, reduce_kernels.hip: slices of 16, four
// chains, slice order): no atomics, the launch shape depends on m only, so the same input gives the same bits on every
// run and at every batch position.
// -ffp-contract=off: each expression below is exactly the float32 operations written, in the order written.
#include <math.h>

#include "sei_common.h"

namespace {

constexpr int DPS_THREADS = 256;
constexpr unsigned DPS_GRID_CAP = 1024;      // partials per image
constexpr int DPS_MAX_B = 65535;             // blockIdx.y

inline unsigned dps_grid(size_t m) { return sei_capped_grid(m / 4, DPS_THREADS, DPS_GRID_CAP); }

inline bool dps_al16(const void *a, const void *b = nullptr, const void *c = nullptr, const void *d = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
             reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

// the four floats from element i on (the tensors are 16-byte aligned, so i % 4 says whether this quad is; uniform per image)
__device__ __forceinline__ float4 ld4(const float *p, size_t i) {
    if ((i & 3) == 0) return *reinterpret_cast<const float4 *>(p + i);
    return make_float4(p[i], p[i + 1], p[i + 2], p[i + 3]);
}
__device__ __forceinline__ void st4(float *p, size_t i, const float4 v) {
    if ((i & 3) == 0) {
        *reinterpret_cast<float4 *>(p + i) = v;
    } else {
        p[i] = v.x; p[i + 1] = v.y; p[i + 2] = v.z; p[i + 3] = v.w;
    }
}

// The frame of every kernel here, for image blockIdx.y of m elements: `quad(i)` for the quads, i the first element of
// each, then `one(i)` for the elements behind the last quad.
template <class Quad, class One>
__device__ __forceinline__ void dps_stream(size_t m, Quad quad, One one) {
    const size_t base = (size_t)blockIdx.y * m;
    const size_t nq = m / 4, stride = (size_t)gridDim.x * DPS_THREADS;
    for (size_t q = (size_t)blockIdx.x * DPS_THREADS + threadIdx.x; q < nq; q += stride) quad(base + 4 * q);
    if (blockIdx.x == 0 && threadIdx.x < m - 4 * nq) one(base + 4 * nq + threadIdx.x);
}

// torch.clamp(2 o - 1, -1, 1), operation by operation (a NaN stays a NaN, as in torch.clamp)
__device__ __forceinline__ float dps_x0(float o) {
    const float t = 2.f * o - 1.f;
    return t < -1.f ? -1.f : (t > 1.f ? 1.f : t);
}
// the clamp's derivative as autograd takes it: 1 on the closed interval
__device__ __forceinline__ bool dps_inside(float o) {
    const float t = 2.f * o - 1.f;
    return t >= -1.f && t <= 1.f;
}

__global__ __launch_bounds__(DPS_THREADS) void dps_u_kernel(const float *__restrict__ out, float *__restrict__ u, size_t m) {
    auto element = [](float o) { return dps_x0(o) / 2.f + 0.5f; };
    dps_stream(
        m,
        [&](size_t i) {
            const float4 o = ld4(out, i);
            st4(u, i, make_float4(element(o.x), element(o.y), element(o.z), element(o.w)));
        },
        [&](size_t i) { u[i] = element(out[i]); });
}

__global__ __launch_bounds__(DPS_THREADS) void dps_residual_kernel(const float *__restrict__ Au, const float *__restrict__ y,
                                                                   float *__restrict__ r, float *__restrict__ part, size_t m) {
    float acc = 0.f;
    auto element = [&](float a, float b) {
        const float v = a - b;
        acc += v * v;
        return v;
    };
    dps_stream(
        m,
        [&](size_t i) {
            const float4 a = ld4(Au, i), b = ld4(y, i);
            st4(r, i, make_float4(element(a.x, b.x), element(a.y, b.y), element(a.z, b.z), element(a.w, b.w)));
        },
        [&](size_t i) { r[i] = element(Au[i], y[i]); });
    __shared__ float scratch[DPS_THREADS / 64];
    const float s = sei_block_sum<DPS_THREADS>(acc, scratch);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = s;
}

// part[groups][B] -> f[b] = 0.5 sum, s[b] = 1 / (2 sqrt(f[b])) or 0: one workgroup of 16 slices x 16 images, the order of
// fold_entries (reduce_kernels.hip) for every image: slice k sums the groups k, k + 16, .. on four chains while four are
// left and the tail into chain 0, the chains pair up (s0 + s1) + (s2 + s3), the slices are added in slice order from 0.f.
constexpr int DPS_FOLD_SLICES = 16, DPS_FOLD_E = 16;
__global__ __launch_bounds__(DPS_FOLD_SLICES * DPS_FOLD_E) void dps_fold_kernel(const float *__restrict__ part, int groups, int B,
                                                                                float *__restrict__ f, float *__restrict__ s) {
    __shared__ float red[DPS_FOLD_SLICES * DPS_FOLD_E];
    const int el = threadIdx.x % DPS_FOLD_E, slice = threadIdx.x / DPS_FOLD_E;
    for (int first = 0; first < B; first += DPS_FOLD_E) {
        const int b = first + el;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        if (b < B) {
            int p = slice;
            for (; p + 48 < groups; p += 64) {
                s0 += part[(size_t)p * B + b];
                s1 += part[(size_t)(p + 16) * B + b];
                s2 += part[(size_t)(p + 32) * B + b];
                s3 += part[(size_t)(p + 48) * B + b];
            }
            for (; p < groups; p += 16) s0 += part[(size_t)p * B + b];
        }
        if (first > 0) __syncthreads();                          // (the last round's read of red)
        red[slice * DPS_FOLD_E + el] = (s0 + s1) + (s2 + s3);
        __syncthreads();
        if (slice == 0 && b < B) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < DPS_FOLD_SLICES; ++k) t += red[k * DPS_FOLD_E + el];
            const float fb = 0.5f * t;
            f[b] = fb;
            s[b] = fb > 0.f ? 1.f / (2.f * sqrtf(fb)) : 0.f;     // (a NaN residual gives 0 too: nothing is propagated)
        }
    }
}

__global__ __launch_bounds__(DPS_THREADS) void dps_seed_kernel(const float *__restrict__ Atr, const float *__restrict__ out,
                                                               float *__restrict__ seed, size_t m) {
    auto element = [](float a, float o) { return dps_inside(o) ? a : 0.f; };
    dps_stream(
        m,
        [&](size_t i) {
            const float4 a = ld4(Atr, i), o = ld4(out, i);
            st4(seed, i, make_float4(element(a.x, o.x), element(a.y, o.y), element(a.z, o.z), element(a.w, o.w)));
        },
        [&](size_t i) { seed[i] = element(Atr[i], out[i]); });
}

struct StepScalars {
    float c0, c1, st, ginv, den;
};

__global__ __launch_bounds__(DPS_THREADS) void dps_step_kernel(const float *__restrict__ out, const float *__restrict__ gx,
                                                               const float *__restrict__ nz, const float *__restrict__ s,
                                                               float *__restrict__ x, float *__restrict__ xin, StepScalars c,
                                                               size_t m) {
    const float gs = c.ginv * s[blockIdx.y];
    auto element = [&](float o, float g, float z, float xi, float &next_in) {
        const float xn = ((c.c0 * dps_x0(o) + c.st * z) + c.c1 * xi) - gs * g;
        next_in = xn / c.den + 0.5f;
        return xn;
    };
    dps_stream(
        m,
        [&](size_t i) {
            const float4 o = ld4(out, i), g = ld4(gx, i), z = ld4(nz, i), xv = ld4(x, i);
            float4 n, in;
            n.x = element(o.x, g.x, z.x, xv.x, in.x);
            n.y = element(o.y, g.y, z.y, xv.y, in.y);
            n.z = element(o.z, g.z, z.z, xv.z, in.z);
            n.w = element(o.w, g.w, z.w, xv.w, in.w);
            st4(x, i, n);
            st4(xin, i, in);
        },
        [&](size_t i) { x[i] = element(out[i], gx[i], nz[i], x[i], xin[i]); });
}

inline bool dps_shape(int B, size_t m) { return B >= 1 && B <= DPS_MAX_B && m > 0 && m < ((size_t)1 << 40); }

}  // namespace

extern "C" size_t sei_dps_partials(int B, size_t m) { return dps_shape(B, m) ? (size_t)dps_grid(m) * B : 0; }

extern "C" int sei_dps_u(const float *out, float *u, int B, size_t m, void *stream) {
    SEI_REQUIRE(out && u && out != u && dps_shape(B, m) && dps_al16(out, u));
    hipLaunchKernelGGL(dps_u_kernel, dim3(dps_grid(m), B), dim3(DPS_THREADS), 0, (hipStream_t)stream, out, u, m);
    return sei_launch_status();
}

extern "C" int sei_dps_residual(const float *Au, const float *y, float *r, float *part, float *f, float *s, int B, size_t m,
                                void *stream) {
    SEI_REQUIRE(Au && y && r && part && f && s && f != s && dps_shape(B, m));
    SEI_REQUIRE(dps_al16(Au, y, r) && ((reinterpret_cast<uintptr_t>(part) | reinterpret_cast<uintptr_t>(f) |
                                        reinterpret_cast<uintptr_t>(s)) & 3) == 0);
    const unsigned grid = dps_grid(m);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(dps_residual_kernel, dim3(grid, B), dim3(DPS_THREADS), 0, st, Au, y, r, part, m);
    if (const int rc = sei_launch_status()) return rc;
    hipLaunchKernelGGL(dps_fold_kernel, dim3(1), dim3(DPS_FOLD_SLICES * DPS_FOLD_E), 0, st, (const float *)part, (int)grid, B, f, s);
    return sei_launch_status();
}

extern "C" int sei_dps_seed(const float *Atr, const float *out, float *seed, int B, size_t m, void *stream) {
    SEI_REQUIRE(Atr && out && seed && dps_shape(B, m) && dps_al16(Atr, out, seed));
    hipLaunchKernelGGL(dps_seed_kernel, dim3(dps_grid(m), B), dim3(DPS_THREADS), 0, (hipStream_t)stream, Atr, out, seed, m);
    return sei_launch_status();
}

extern "C" int sei_dps_step(const float *out, const float *gx, const float *nz, const float *s, float *x, float *xin, float c0,
                            float c1, float st, float ginv, float den, int B, size_t m, void *stream) {
    SEI_REQUIRE(out && gx && nz && s && x && xin && dps_shape(B, m));
    SEI_REQUIRE(out != x && gx != x && nz != x && xin != x);
    SEI_REQUIRE(isfinite(c0) && isfinite(c1) && isfinite(st) && isfinite(ginv) && isfinite(den) && den > 0.f);
    SEI_REQUIRE(dps_al16(out, gx, nz, x) && dps_al16(xin) && (reinterpret_cast<uintptr_t>(s) & 3) == 0);
    const StepScalars c{c0, c1, st, ginv, den};
    hipLaunchKernelGGL(dps_step_kernel, dim3(dps_grid(m), B), dim3(DPS_THREADS), 0, (hipStream_t)stream, out, gx, nz, s, x, xin, c,
                       m);
    return sei_launch_status();
}
