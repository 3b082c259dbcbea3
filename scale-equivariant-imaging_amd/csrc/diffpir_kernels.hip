// The data step and the sampling step of the DiffPIR baseline for gfx950, float32 (models/diffpir.py, models/_cg.py;
// deepinv v0.2.0's DiffPIR.forward and optim.utils.conjugate_gradient restated).
//
//   sei_cg_init / _apply / _update / _direction : conjugate gradients on (A^T A + I / gamma) u = A^T y + u0 / gamma from zero.
//       Every scalar of the solve (rs, pAp, rs_new, the stopping flag, the iteration count) lives in a SeiCgState on the
//       device; the kernels read it and the one-workgroup fold behind each reduction writes it, so no scalar crosses to
//       the host inside an iteration. A^T A p itself comes from the physics' own kernels between _direction and _apply.
//   sei_diffpir_sample : one pass from the prox result to the next iterate and the next denoiser input.
//
// All of them stream flat tensors of n >= 1 floats: 16-byte lanes over the n / 4 quads (grid stride), the n % 4 tail
// elements by the first lanes of workgroup 0. A reducing kernel leaves one partial per workgroup (a fixed shuffle tree over
// per-thread sums taken in index order) and sei_fold_cg (reduce_kernels.hip) adds the partials in the order of every
// fold of this library: no atomics, the launch shape depends on n only, so the same input gives the same bits every run.
// -ffp-contract=off: each expression below is exactly the float32 operations written, in the order written.
#include <math.h>

#include "sei_common.h"

namespace {

constexpr int CG_THREADS = 256;
constexpr unsigned CG_GRID_CAP = 1024;       // partials per reduction: one fold workgroup adds them in a few dozen steps

inline unsigned cg_grid(size_t n) { return sei_capped_grid(n / 4, CG_THREADS, CG_GRID_CAP); }

inline bool aligned16(const void *a, const void *b = nullptr, const void *c = nullptr, const void *d = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
             reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

__device__ __forceinline__ float4 ld4(const float *p, size_t q) { return reinterpret_cast<const float4 *>(p)[q]; }
__device__ __forceinline__ void st4(float *p, size_t q, const float4 v) { reinterpret_cast<float4 *>(p)[q] = v; }

// The frame of every kernel here: `quad(q)` for the quads in grid-stride order, then `tail(i)` for the elements behind
// the last quad (workgroup 0, one lane each).
template <class Quad, class Tail>
__device__ __forceinline__ void cg_stream(size_t n, Quad quad, Tail tail) {
    const size_t nq = n / 4, stride = (size_t)gridDim.x * CG_THREADS;
    for (size_t q = (size_t)blockIdx.x * CG_THREADS + threadIdx.x; q < nq; q += stride) quad(q);
    if (blockIdx.x == 0 && threadIdx.x < n - 4 * nq) tail(4 * nq + threadIdx.x);
}

__device__ __forceinline__ void cg_partial(float acc, float *__restrict__ part) {
    __shared__ float scratch[CG_THREADS / 64];
    const float s = sei_block_sum<CG_THREADS>(acc, scratch);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// torch.clamp(2 o - 1, -1, 1) / 2 + 0.5, operation by operation (a NaN stays a NaN, as in torch.clamp)
__device__ __forceinline__ float diffpir_prologue(float o) {
    float t = 2.f * o - 1.f;
    t = t < -1.f ? -1.f : (t > 1.f ? 1.f : t);
    return t / 2.f + 0.5f;
}

template <bool PROLOGUE>
__global__ __launch_bounds__(CG_THREADS) void cg_init_kernel(const float *__restrict__ u0, const float *__restrict__ Aty,
                                                             float inv_gamma, float *__restrict__ x, float *__restrict__ r,
                                                             float *__restrict__ p, float *__restrict__ part, size_t n) {
    float acc = 0.f;
    auto element = [&](float u, float a) {
        if (PROLOGUE) u = diffpir_prologue(u);
        const float b = a + u * inv_gamma;
        acc += b * b;
        return b;
    };
    cg_stream(
        n,
        [&](size_t q) {
            const float4 u = ld4(u0, q), a = ld4(Aty, q);
            const float4 b = make_float4(element(u.x, a.x), element(u.y, a.y), element(u.z, a.z), element(u.w, a.w));
            st4(x, q, make_float4(0.f, 0.f, 0.f, 0.f));
            st4(r, q, b);
            st4(p, q, b);
        },
        [&](size_t i) {
            const float b = element(u0[i], Aty[i]);
            x[i] = 0.f;
            r[i] = b;
            p[i] = b;
        });
    cg_partial(acc, part);
}

__global__ __launch_bounds__(CG_THREADS) void cg_apply_kernel(const float *__restrict__ p, const float *__restrict__ AtAp,
                                                              float inv_gamma, float *__restrict__ Ap,
                                                              float *__restrict__ part, const SeiCgState *__restrict__ st,
                                                              size_t n) {
    if (st->done) return;
    float acc = 0.f;
    auto element = [&](float pi, float ai) {
        const float v = ai + pi * inv_gamma;
        acc += pi * v;
        return v;
    };
    cg_stream(
        n,
        [&](size_t q) {
            const float4 pv = ld4(p, q), av = ld4(AtAp, q);
            st4(Ap, q, make_float4(element(pv.x, av.x), element(pv.y, av.y), element(pv.z, av.z), element(pv.w, av.w)));
        },
        [&](size_t i) { Ap[i] = element(p[i], AtAp[i]); });
    cg_partial(acc, part);
}

__global__ __launch_bounds__(CG_THREADS) void cg_update_kernel(float *__restrict__ x, float *__restrict__ r,
                                                               const float *__restrict__ p, const float *__restrict__ Ap,
                                                               float *__restrict__ part, const SeiCgState *__restrict__ st,
                                                               size_t n) {
    if (st->done) return;
    const float alpha = st->rs / st->pAp;
    float acc = 0.f;
    auto residual = [&](float ri, float ai) {
        const float v = ri - alpha * ai;
        acc += v * v;
        return v;
    };
    cg_stream(
        n,
        [&](size_t q) {
            const float4 xv = ld4(x, q), rv = ld4(r, q), pv = ld4(p, q), av = ld4(Ap, q);
            st4(x, q, make_float4(xv.x + alpha * pv.x, xv.y + alpha * pv.y, xv.z + alpha * pv.z, xv.w + alpha * pv.w));
            st4(r, q, make_float4(residual(rv.x, av.x), residual(rv.y, av.y), residual(rv.z, av.z), residual(rv.w, av.w)));
        },
        [&](size_t i) {
            x[i] = x[i] + alpha * p[i];
            r[i] = residual(r[i], Ap[i]);
        });
    cg_partial(acc, part);
}

// beta = rs_new / rs, divided by the fold behind sei_cg_update, which then made rs = rs_new: this launch writes no state.
__global__ __launch_bounds__(CG_THREADS) void cg_direction_kernel(float *__restrict__ p, const float *__restrict__ r,
                                                                  const SeiCgState *__restrict__ st, size_t n) {
    if (st->done) return;
    const float beta = st->beta;
    cg_stream(
        n,
        [&](size_t q) {
            const float4 pv = ld4(p, q), rv = ld4(r, q);
            st4(p, q, make_float4(rv.x + pv.x * beta, rv.y + pv.y * beta, rv.z + pv.z * beta, rv.w + pv.w * beta));
        },
        [&](size_t i) { p[i] = r[i] + p[i] * beta; });
}

struct SampleScalars {
    float sa_t, s1m_t, sa_n, s1m_n, c_eps, c_nz, den;
};

__global__ __launch_bounds__(CG_THREADS) void diffpir_sample_kernel(const float *__restrict__ u, float *__restrict__ x,
                                                                    const float *__restrict__ nz, float *__restrict__ xin,
                                                                    SampleScalars c, size_t n) {
    auto element = [&](float ui, float xi, float zi, float &next_in) {
        const float x0 = 2.f * ui - 1.f;
        const float eps = (xi - c.sa_t * x0) / c.s1m_t;
        const float xn = c.sa_n * x0 + c.s1m_n * (c.c_eps * eps + c.c_nz * zi);
        next_in = xn / c.den + 0.5f;
        return xn;
    };
    cg_stream(
        n,
        [&](size_t q) {
            const float4 uv = ld4(u, q), xv = ld4(x, q), zv = ld4(nz, q);
            float4 o, in;
            o.x = element(uv.x, xv.x, zv.x, in.x);
            o.y = element(uv.y, xv.y, zv.y, in.y);
            o.z = element(uv.z, xv.z, zv.z, in.z);
            o.w = element(uv.w, xv.w, zv.w, in.w);
            st4(x, q, o);
            st4(xin, q, in);
        },
        [&](size_t i) { x[i] = element(u[i], x[i], nz[i], xin[i]); });
}

}  // namespace

extern "C" size_t sei_cg_partials(size_t n) { return n == 0 ? 0 : cg_grid(n); }

extern "C" int sei_cg_init(const float *u0, const float *Aty, float inv_gamma, int prologue, float *x, float *r, float *p,
                           float *part, SeiCgState *state, size_t n, void *stream) {
    SEI_REQUIRE(u0 && Aty && x && r && p && part && state && n > 0);
    SEI_REQUIRE(isfinite(inv_gamma) && (prologue == 0 || prologue == 1));
    SEI_REQUIRE(aligned16(u0, Aty, x, r) && aligned16(p) && (reinterpret_cast<uintptr_t>(state) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(part) & 3) == 0);
    const unsigned grid = cg_grid(n);
    hipStream_t s = (hipStream_t)stream;
    if (prologue)
        hipLaunchKernelGGL(cg_init_kernel<true>, dim3(grid), dim3(CG_THREADS), 0, s, u0, Aty, inv_gamma, x, r, p, part, n);
    else
        hipLaunchKernelGGL(cg_init_kernel<false>, dim3(grid), dim3(CG_THREADS), 0, s, u0, Aty, inv_gamma, x, r, p, part, n);
    if (const int rc = sei_launch_status()) return rc;
    return sei_fold_cg(part, (int)grid, state, SEI_CG_FOLD_RS, 0.f, s);
}

extern "C" int sei_cg_apply(const float *p, const float *AtAp, float inv_gamma, float *Ap, float *part, SeiCgState *state,
                            size_t n, void *stream) {
    SEI_REQUIRE(p && AtAp && Ap && part && state && n > 0 && isfinite(inv_gamma));
    SEI_REQUIRE(aligned16(p, AtAp, Ap) && (reinterpret_cast<uintptr_t>(state) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(part) & 3) == 0);
    const unsigned grid = cg_grid(n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cg_apply_kernel, dim3(grid), dim3(CG_THREADS), 0, s, p, AtAp, inv_gamma, Ap, part, state, n);
    if (const int rc = sei_launch_status()) return rc;
    return sei_fold_cg(part, (int)grid, state, SEI_CG_FOLD_PAP, 0.f, s);
}

extern "C" int sei_cg_update(float *x, float *r, const float *p, const float *Ap, float tol, float *part, SeiCgState *state,
                             size_t n, void *stream) {
    SEI_REQUIRE(x && r && p && Ap && part && state && n > 0 && tol >= 0.f && isfinite(tol));
    SEI_REQUIRE(aligned16(x, r, p, Ap) && (reinterpret_cast<uintptr_t>(state) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(part) & 3) == 0);
    const unsigned grid = cg_grid(n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cg_update_kernel, dim3(grid), dim3(CG_THREADS), 0, s, x, r, p, Ap, part, state, n);
    if (const int rc = sei_launch_status()) return rc;
    return sei_fold_cg(part, (int)grid, state, SEI_CG_FOLD_RS_NEW, tol, s);
}

extern "C" int sei_cg_direction(float *p, const float *r, const SeiCgState *state, size_t n, void *stream) {
    SEI_REQUIRE(p && r && state && n > 0);
    SEI_REQUIRE(aligned16(p, r) && (reinterpret_cast<uintptr_t>(state) & 3) == 0);
    hipLaunchKernelGGL(cg_direction_kernel, dim3(cg_grid(n)), dim3(CG_THREADS), 0, (hipStream_t)stream, p, r, state, n);
    return sei_launch_status();
}

extern "C" int sei_diffpir_sample(const float *u, float *x, const float *nz, float *xin, float sa_t, float s1m_t, float sa_n,
                                  float s1m_n, float zeta, float at_n, size_t n, void *stream) {
    SEI_REQUIRE(u && x && nz && xin && n > 0);
    SEI_REQUIRE(isfinite(sa_t) && isfinite(sa_n) && isfinite(s1m_n) && isfinite(s1m_t) && s1m_t != 0.f);
    SEI_REQUIRE(zeta >= 0.f && zeta <= 1.f && at_n > 0.f && isfinite(at_n));
    SEI_REQUIRE(aligned16(u, x, nz, xin));
    SampleScalars c;
    c.sa_t = sa_t; c.s1m_t = s1m_t; c.sa_n = sa_n; c.s1m_n = s1m_n;
    c.c_eps = (float)sqrt(1.0 - (double)zeta);
    c.c_nz = (float)sqrt((double)zeta);
    c.den = (float)(2.0 * sqrt((double)at_n));
    hipLaunchKernelGGL(diffpir_sample_kernel, dim3(cg_grid(n)), dim3(CG_THREADS), 0, (hipStream_t)stream, u, x, nz, xin, c, n);
    return sei_launch_status();
}
