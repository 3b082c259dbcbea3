// LayerNorm over the channel axis for gfx950 (reference: src/models/convolutional.py:21-30), NHWC float32.
//
//   sei_ln_fwd / sei_ln_bwd / sei_ln_bwd_res : LayerNorm over channels, eps 1e-6, biased variance
//
// HBM-bound streaming kernels: channels are the contiguous axis, so lanes map to channels and every global access is a
// coalesced 256-B wave row. The parameter gradients of the vectorised shapes are per-workgroup partial rows, folded in a
// fixed order by sei_fold_now or sei_fold_many (reduce_kernels.hip); the legacy shapes add with float atomics after
// an in-block LDS reduction (gradients are accumulators by contract).
#include "sei_common.h"

namespace {

constexpr int LN_THREADS = 256;
constexpr int LN_EPL = 8;   // max elements per lane in the group kernels (C <= G*LN_EPL)

// G lanes per row, C <= 8*G. Row data lives in registers (one HBM read), statistics by shuffles.
template <int G>
__global__ __launch_bounds__(LN_THREADS) void ln_fwd_group_kernel(
    const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
    float *__restrict__ y, float *__restrict__ mean, float *__restrict__ rstd, size_t rows, int C, float eps) {
    const int lg = threadIdx.x % G, rsub = threadIdx.x / G;
    constexpr int RPB = LN_THREADS / G;
    const float invC = 1.0f / (float)C;
    for (size_t row = (size_t)blockIdx.x * RPB + rsub; row < rows; row += (size_t)gridDim.x * RPB) {
        const float *xr = x + row * C;
        float v[LN_EPL];
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < LN_EPL; ++e) {
            const int c = lg + e * G;
            v[e] = c < C ? xr[c] : 0.f;
            s += v[e];
        }
        const float mu = sei_group_sum<G>(s) * invC;
        float q = 0.f;
#pragma unroll
        for (int e = 0; e < LN_EPL; ++e) {
            const int c = lg + e * G;
            const float d = c < C ? v[e] - mu : 0.f;
            q = fmaf(d, d, q);
        }
        const float rs = 1.0f / sqrtf(sei_group_sum<G>(q) * invC + eps);
        float *yr = y + row * C;
#pragma unroll
        for (int e = 0; e < LN_EPL; ++e) {
            const int c = lg + e * G;
            if (c < C) yr[c] = fmaf((v[e] - mu) * rs, gamma[c], beta[c]);
        }
        if (lg == 0) {
            mean[row] = mu;
            rstd[row] = rs;
        }
    }
}

// One workgroup per row for wide rows: element c = tid + k*256, up to LN_WIDE_EPT per thread.
constexpr int LN_WIDE_EPT = 32;   // C <= 8192
__global__ __launch_bounds__(LN_THREADS) void ln_fwd_wide_kernel(
    const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
    float *__restrict__ y, float *__restrict__ mean, float *__restrict__ rstd, size_t rows, int C, float eps) {
    __shared__ float scratch[LN_THREADS / 64];
    __shared__ float bc[2];
    const float invC = 1.0f / (float)C;
    for (size_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const float *xr = x + row * C;
        float v[LN_WIDE_EPT];
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < LN_WIDE_EPT; ++e) {
            const int c = threadIdx.x + e * LN_THREADS;
            v[e] = c < C ? xr[c] : 0.f;
            s += v[e];
        }
        s = sei_block_sum<LN_THREADS>(s, scratch);
        if (threadIdx.x == 0) bc[0] = s * invC;
        __syncthreads();
        const float mu = bc[0];
        float q = 0.f;
#pragma unroll
        for (int e = 0; e < LN_WIDE_EPT; ++e) {
            const int c = threadIdx.x + e * LN_THREADS;
            const float d = c < C ? v[e] - mu : 0.f;
            q = fmaf(d, d, q);
        }
        q = sei_block_sum<LN_THREADS>(q, scratch);
        if (threadIdx.x == 0) bc[1] = 1.0f / sqrtf(q * invC + eps);
        __syncthreads();
        const float rs = bc[1];
        float *yr = y + row * C;
#pragma unroll
        for (int e = 0; e < LN_WIDE_EPT; ++e) {
            const int c = threadIdx.x + e * LN_THREADS;
            if (c < C) yr[c] = fmaf((v[e] - mu) * rs, gamma[c], beta[c]);
        }
        if (threadIdx.x == 0) {
            mean[row] = mu;
            rstd[row] = rs;
        }
        __syncthreads();
    }
}

// backward: gx = rstd * (g - mean(g) - xhat * mean(g*xhat)), g = gy*gamma;
//           ggamma[c] += sum_rows gy*xhat; gbeta[c] += sum_rows gy.
template <int G>
__global__ __launch_bounds__(LN_THREADS) void ln_bwd_group_kernel(
    const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ mean,
    const float *__restrict__ rstd, const float *__restrict__ gy, float *__restrict__ gx,
    float *__restrict__ ggamma, float *__restrict__ gbeta, size_t rows, int C) {
    extern __shared__ __attribute__((aligned(16))) float smem[];   // [2][C]
    const int lg = threadIdx.x % G, rsub = threadIdx.x / G;
    constexpr int RPB = LN_THREADS / G;
    for (int e = threadIdx.x; e < 2 * C; e += LN_THREADS) smem[e] = 0.f;
    __syncthreads();
    const float invC = 1.0f / (float)C;
    float gam[LN_EPL], dg[LN_EPL], db[LN_EPL];
#pragma unroll
    for (int e = 0; e < LN_EPL; ++e) {
        const int c = lg + e * G;
        gam[e] = c < C ? gamma[c] : 0.f;
        dg[e] = 0.f;
        db[e] = 0.f;
    }
    for (size_t row = (size_t)blockIdx.x * RPB + rsub; row < rows; row += (size_t)gridDim.x * RPB) {
        const float mu = mean[row], rs = rstd[row];
        const float *xr = x + row * C, *gr = gy + row * C;
        float xh[LN_EPL], g[LN_EPL];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < LN_EPL; ++e) {
            const int c = lg + e * G;
            const float gyv = c < C ? gr[c] : 0.f;
            xh[e] = c < C ? (xr[c] - mu) * rs : 0.f;
            g[e] = gyv * gam[e];
            s1 += g[e];
            s2 = fmaf(g[e], xh[e], s2);
            dg[e] = fmaf(gyv, xh[e], dg[e]);
            db[e] += gyv;
        }
        s1 = sei_group_sum<G>(s1) * invC;
        s2 = sei_group_sum<G>(s2) * invC;
        float *gxr = gx + row * C;
#pragma unroll
        for (int e = 0; e < LN_EPL; ++e) {
            const int c = lg + e * G;
            if (c < C) gxr[c] = rs * (g[e] - s1 - xh[e] * s2);
        }
    }
#pragma unroll
    for (int e = 0; e < LN_EPL; ++e) {
        const int c = lg + e * G;
        if (c < C) {
            atomicAdd(&smem[c], dg[e]);
            atomicAdd(&smem[C + c], db[e]);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += LN_THREADS) {
        atomicAdd(ggamma + c, smem[c]);
        atomicAdd(gbeta + c, smem[C + c]);
    }
}

__global__ __launch_bounds__(LN_THREADS) void ln_bwd_wide_kernel(
    const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ mean,
    const float *__restrict__ rstd, const float *__restrict__ gy, float *__restrict__ gx,
    float *__restrict__ ggamma, float *__restrict__ gbeta, size_t rows, int C) {
    __shared__ float scratch[LN_THREADS / 64];
    __shared__ float bc[2];
    const float invC = 1.0f / (float)C;
    float gam[LN_WIDE_EPT], dg[LN_WIDE_EPT], db[LN_WIDE_EPT];
#pragma unroll
    for (int e = 0; e < LN_WIDE_EPT; ++e) {
        const int c = threadIdx.x + e * LN_THREADS;
        gam[e] = c < C ? gamma[c] : 0.f;
        dg[e] = 0.f;
        db[e] = 0.f;
    }
    for (size_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const float mu = mean[row], rs = rstd[row];
        const float *xr = x + row * C, *gr = gy + row * C;
        float xh[LN_WIDE_EPT], g[LN_WIDE_EPT];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < LN_WIDE_EPT; ++e) {
            const int c = threadIdx.x + e * LN_THREADS;
            const float gyv = c < C ? gr[c] : 0.f;
            xh[e] = c < C ? (xr[c] - mu) * rs : 0.f;
            g[e] = gyv * gam[e];
            s1 += g[e];
            s2 = fmaf(g[e], xh[e], s2);
            dg[e] = fmaf(gyv, xh[e], dg[e]);
            db[e] += gyv;
        }
        s1 = sei_block_sum<LN_THREADS>(s1, scratch);
        s2 = sei_block_sum<LN_THREADS>(s2, scratch);
        if (threadIdx.x == 0) {
            bc[0] = s1 * invC;
            bc[1] = s2 * invC;
        }
        __syncthreads();
        const float m1 = bc[0], m2 = bc[1];
        float *gxr = gx + row * C;
#pragma unroll
        for (int e = 0; e < LN_WIDE_EPT; ++e) {
            const int c = threadIdx.x + e * LN_THREADS;
            if (c < C) gxr[c] = rs * (g[e] - m1 - xh[e] * m2);
        }
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < LN_WIDE_EPT; ++e) {
        const int c = threadIdx.x + e * LN_THREADS;
        if (c < C) {
            atomicAdd(ggamma + c, dg[e]);
            atomicAdd(gbeta + c, db[e]);
        }
    }
}

// ---- LayerNorm backward, vectorised (C % 4 == 0) -----------------------------------------------------------
// Parameter gradients are written as per-workgroup partial rows into a workspace and folded in the fixed order of
// reduce_kernels.hip (no atomics, bitwise reproducible).
//
// narrow rows (C = 4*G*NV, G a power of two <= 64): G lanes own one row, NV float4 each; 256/G rows per sweep.
template <int G, int NV>
__global__ __launch_bounds__(LN_THREADS) void ln_bwd_vec_kernel(
    const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ mean,
    const float *__restrict__ rstd, const float *__restrict__ gy, const float *__restrict__ res,
    float *__restrict__ gx, float *__restrict__ part, size_t rows) {
    constexpr int C = 4 * G * NV, RPB = LN_THREADS / G;
    __shared__ __attribute__((aligned(16))) float red[RPB * 2 * C];
    const int lg = threadIdx.x % G, rsub = threadIdx.x / G;
    const float invC = 1.0f / (float)C;
    float4 gam[NV], dg[NV], db[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        gam[e] = *reinterpret_cast<const float4 *>(gamma + 4 * (lg + e * G));
        dg[e] = db[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (size_t row = (size_t)blockIdx.x * RPB + rsub; row < rows; row += (size_t)gridDim.x * RPB) {
        const float mu = mean[row], rs = rstd[row];
        float4 xh[NV], g[NV];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const size_t o = row * C + 4 * (lg + e * G);
            const float4 xv = *reinterpret_cast<const float4 *>(x + o);
            const float4 gv = *reinterpret_cast<const float4 *>(gy + o);
#define SEI_LN_BWD_LANE(f)                              \
    xh[e].f = (xv.f - mu) * rs;                         \
    g[e].f = gv.f * gam[e].f;                           \
    s1 += g[e].f;                                       \
    s2 = fmaf(g[e].f, xh[e].f, s2);                     \
    dg[e].f = fmaf(gv.f, xh[e].f, dg[e].f);             \
    db[e].f += gv.f;
            SEI_LN_BWD_LANE(x) SEI_LN_BWD_LANE(y) SEI_LN_BWD_LANE(z) SEI_LN_BWD_LANE(w)
#undef SEI_LN_BWD_LANE
        }
        s1 = sei_group_sum<G>(s1) * invC;
        s2 = sei_group_sum<G>(s2) * invC;
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            float4 o4;
            o4.x = rs * (g[e].x - s1 - xh[e].x * s2);
            o4.y = rs * (g[e].y - s1 - xh[e].y * s2);
            o4.z = rs * (g[e].z - s1 - xh[e].z * s2);
            o4.w = rs * (g[e].w - s1 - xh[e].w * s2);
            if (res) {                                           // a second gradient of the same tensor (skip connection)
                const float4 r4 = *reinterpret_cast<const float4 *>(res + row * C + 4 * (lg + e * G));
                o4.x += r4.x; o4.y += r4.y; o4.z += r4.z; o4.w += r4.w;
            }
            *reinterpret_cast<float4 *>(gx + row * C + 4 * (lg + e * G)) = o4;
        }
    }
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        *reinterpret_cast<float4 *>(red + (rsub * 2 + 0) * C + 4 * (lg + e * G)) = dg[e];
        *reinterpret_cast<float4 *>(red + (rsub * 2 + 1) * C + 4 * (lg + e * G)) = db[e];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * C; e += LN_THREADS) {
        float s = 0.f;
#pragma unroll 4
        for (int r = 0; r < RPB; ++r) s += red[r * 2 * C + e];
        part[(size_t)blockIdx.x * 2 * C + e] = s;
    }
}

// wide rows in ONE pass (C = 1024 NV, NV <= 8; round 5): a workgroup takes whole rows -- a thread owns NV float4 of the row,
// 1 KiB apart, so x and gy are read ONCE (the two-pass form below reads both twice: 565 MB per 113-MB tensor where this one
// moves 340 MB + the partials) --, folds the row's two sums over its four waves through LDS, writes gx, and keeps the
// parameter-gradient partials of ITS rows in registers: part[workgroup][2 C] for sei_fold_many / sei_fold_now.
// The next row's loads are issued before the current row's sums are exchanged.
template <int NV>
__global__ __launch_bounds__(LN_THREADS) void ln_bwd_row_kernel(
    const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ mean,
    const float *__restrict__ rstd, const float *__restrict__ gy, const float *__restrict__ res,
    float *__restrict__ gx, float *__restrict__ part, size_t rows) {
    constexpr int C = 1024 * NV;
    __shared__ float red[2][2][LN_THREADS / 64];               // [row parity][sum][wave]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float invC = 1.0f / (float)C;
    float4 gam[NV], dg[NV], db[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        gam[e] = *reinterpret_cast<const float4 *>(gamma + 4 * (threadIdx.x + e * LN_THREADS));
        dg[e] = db[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4 xv[NV], gv[NV], xn[NV], gn[NV];
    size_t row = blockIdx.x;
    if (row < rows) {
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const size_t o = row * C + 4 * (threadIdx.x + e * LN_THREADS);
            xn[e] = *reinterpret_cast<const float4 *>(x + o);
            gn[e] = *reinterpret_cast<const float4 *>(gy + o);
        }
    }
    int parity = 0;
    for (; row < rows; row += gridDim.x, parity ^= 1) {
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            xv[e] = xn[e];
            gv[e] = gn[e];
        }
        const size_t next = row + gridDim.x;
        if (next < rows) {
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                const size_t o = next * C + 4 * (threadIdx.x + e * LN_THREADS);
                xn[e] = *reinterpret_cast<const float4 *>(x + o);
                gn[e] = *reinterpret_cast<const float4 *>(gy + o);
            }
        }
        const float mu = mean[row], rs = rstd[row];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < NV; ++e) {
#define SEI_LN_ROW_LANE(f)                               \
    xv[e].f = (xv[e].f - mu) * rs;                       \
    dg[e].f = fmaf(gv[e].f, xv[e].f, dg[e].f);           \
    db[e].f += gv[e].f;                                  \
    gv[e].f *= gam[e].f;                                 \
    s1 += gv[e].f;                                       \
    s2 = fmaf(gv[e].f, xv[e].f, s2);
            SEI_LN_ROW_LANE(x) SEI_LN_ROW_LANE(y) SEI_LN_ROW_LANE(z) SEI_LN_ROW_LANE(w)
#undef SEI_LN_ROW_LANE
        }
        s1 = sei_wave_sum(s1);
        s2 = sei_wave_sum(s2);
        if (lane == 0) {
            red[parity][0][wave] = s1;
            red[parity][1][wave] = s2;
        }
        __syncthreads();                                         // (the other parity's words are free: two barriers back)
        s1 = s2 = 0.f;
#pragma unroll
        for (int k = 0; k < LN_THREADS / 64; ++k) {
            s1 += red[parity][0][k];
            s2 += red[parity][1][k];
        }
        s1 *= invC;
        s2 *= invC;
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const size_t o = row * C + 4 * (threadIdx.x + e * LN_THREADS);
            float4 o4;
            o4.x = rs * (gv[e].x - s1 - xv[e].x * s2);
            o4.y = rs * (gv[e].y - s1 - xv[e].y * s2);
            o4.z = rs * (gv[e].z - s1 - xv[e].z * s2);
            o4.w = rs * (gv[e].w - s1 - xv[e].w * s2);
            if (res) {
                const float4 r4 = *reinterpret_cast<const float4 *>(res + o);
                o4.x += r4.x; o4.y += r4.y; o4.z += r4.z; o4.w += r4.w;
            }
            *reinterpret_cast<float4 *>(gx + o) = o4;
        }
    }
    float *out = part + (size_t)blockIdx.x * 2 * C;
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        *reinterpret_cast<float4 *>(out + 4 * (threadIdx.x + e * LN_THREADS)) = dg[e];
        *reinterpret_cast<float4 *>(out + C + 4 * (threadIdx.x + e * LN_THREADS)) = db[e];
    }
}

// wide rows, pass 1: stats[row] = (mean_c(gy*gamma), mean_c(gy*gamma*xhat)); one workgroup per row.
__global__ __launch_bounds__(LN_THREADS) void ln_bwd_rowstats_kernel(
    const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ mean,
    const float *__restrict__ rstd, const float *__restrict__ gy, float2 *__restrict__ stats, int C) {
    __shared__ float scratch[2][LN_THREADS / 64];
    const size_t row = blockIdx.x;
    const float mu = mean[row], rs = rstd[row];
    float s1 = 0.f, s2 = 0.f;
    for (int c = 4 * threadIdx.x; c < C; c += 4 * LN_THREADS) {
        const float4 xv = *reinterpret_cast<const float4 *>(x + row * C + c);
        const float4 gv = *reinterpret_cast<const float4 *>(gy + row * C + c);
        const float4 gm = *reinterpret_cast<const float4 *>(gamma + c);
        float g;
        g = gv.x * gm.x; s1 += g; s2 = fmaf(g, (xv.x - mu) * rs, s2);
        g = gv.y * gm.y; s1 += g; s2 = fmaf(g, (xv.y - mu) * rs, s2);
        g = gv.z * gm.z; s1 += g; s2 = fmaf(g, (xv.z - mu) * rs, s2);
        g = gv.w * gm.w; s1 += g; s2 = fmaf(g, (xv.w - mu) * rs, s2);
    }
    s1 = sei_wave_sum(s1);
    s2 = sei_wave_sum(s2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        scratch[0][wave] = s1;
        scratch[1][wave] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int k = 0; k < LN_THREADS / 64; ++k) {
            a += scratch[0][k];
            b += scratch[1][k];
        }
        const float invC = 1.0f / (float)C;
        stats[row] = make_float2(a * invC, b * invC);
    }
}

// wide rows, pass 2: a thread owns 4 consecutive channels and walks a chunk of rows (row scalars are
// wave-uniform); gx elementwise, the parameter-gradient partial of the chunk in registers.
__global__ __launch_bounds__(LN_THREADS) void ln_bwd_cols_kernel(
    const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ mean,
    const float *__restrict__ rstd, const float *__restrict__ gy, const float2 *__restrict__ stats,
    const float *__restrict__ res, float *__restrict__ gx, float *__restrict__ part, size_t rows, int C,
    int rows_per_chunk) {
    const int c = 4 * (blockIdx.x * LN_THREADS + threadIdx.x);
    if (c >= C) return;
    const float4 gm = *reinterpret_cast<const float4 *>(gamma + c);
    float4 dg = make_float4(0.f, 0.f, 0.f, 0.f), db = dg;
    const size_t r0 = (size_t)blockIdx.y * rows_per_chunk, r1 = min(rows, r0 + rows_per_chunk);
#pragma unroll 4
    for (size_t row = r0; row < r1; ++row) {
        const float mu = mean[row], rs = rstd[row];
        const float2 st = stats[row];
        const float4 xv = *reinterpret_cast<const float4 *>(x + row * C + c);
        const float4 gv = *reinterpret_cast<const float4 *>(gy + row * C + c);
        float4 o4;
#define SEI_LN_COL_LANE(f)                                   \
    {                                                        \
        const float xh = (xv.f - mu) * rs;                   \
        o4.f = rs * (gv.f * gm.f - st.x - xh * st.y);        \
        dg.f = fmaf(gv.f, xh, dg.f);                         \
        db.f += gv.f;                                        \
    }
        SEI_LN_COL_LANE(x) SEI_LN_COL_LANE(y) SEI_LN_COL_LANE(z) SEI_LN_COL_LANE(w)
#undef SEI_LN_COL_LANE
        if (res) {
            const float4 r4 = *reinterpret_cast<const float4 *>(res + row * C + c);
            o4.x += r4.x; o4.y += r4.y; o4.z += r4.z; o4.w += r4.w;
        }
        *reinterpret_cast<float4 *>(gx + row * C + c) = o4;
    }
    float *out = part + (size_t)blockIdx.y * 2 * C;
    *reinterpret_cast<float4 *>(out + c) = dg;
    *reinterpret_cast<float4 *>(out + C + c) = db;
}

template <int G>
int launch_ln_fwd(const float *x, const float *gamma, const float *beta, float *y, float *mean, float *rstd,
                  size_t rows, int C, float eps, hipStream_t s) {
    const unsigned grid = sei_capped_grid(rows, LN_THREADS / G, 4096);
    hipLaunchKernelGGL(ln_fwd_group_kernel<G>, dim3(grid), dim3(LN_THREADS), 0, s, x, gamma, beta, y, mean, rstd,
                       rows, C, eps);
    return sei_launch_status();
}
template <int G>
int launch_ln_bwd(const float *x, const float *gamma, const float *mean, const float *rstd, const float *gy,
                  float *gx, float *ggamma, float *gbeta, size_t rows, int C, hipStream_t s) {
    // few blocks, many rows each: keeps the global atomics per column low
    const unsigned grid = sei_capped_grid(rows, (LN_THREADS / G) * 4, 1024);
    hipLaunchKernelGGL(ln_bwd_group_kernel<G>, dim3(grid), dim3(LN_THREADS), sizeof(float) * 2 * C, s, x, gamma,
                       mean, rstd, gy, gx, ggamma, gbeta, rows, C);
    return sei_launch_status();
}
inline int ln_group(int C) {
    int g = 1;
    while (g < 64 && g < C) g <<= 1;   // consecutive lanes = consecutive channels
    return g;
}
}  // namespace

__attribute__((visibility("hidden"))) int sei_ln_fwd_f32_lanes16(const float *x, const float *gamma, const float *beta, float *y,
                                                                 float *mean, float *rstd, size_t rows, int C, float eps,
                                                                 hipStream_t s);                  // bf16_support.hip

extern "C" int sei_ln_fwd(const float *x, const float *gamma, const float *beta, float *y, float *mean,
                          float *rstd, size_t rows, int C, float eps, void *stream) {
    SEI_REQUIRE(x && gamma && beta && y && mean && rstd && rows > 0 && C > 0);
    if (C > LN_WIDE_EPT * LN_THREADS) return SEI_ERR_TOO_LARGE;
    hipStream_t s = (hipStream_t)stream;
    {   // 16-byte lanes where the shape allows (C = 4 * 2^k up to 512, any multiple of 4 above)
        const int rc = sei_ln_fwd_f32_lanes16(x, gamma, beta, y, mean, rstd, rows, C, eps, s);
        if (rc >= 0) return rc;
    }
    if (C > 64 * LN_EPL) {
        hipLaunchKernelGGL(ln_fwd_wide_kernel, dim3(sei_capped_grid(rows, 1, 8192)), dim3(LN_THREADS), 0, s, x, gamma,
                           beta, y, mean, rstd, rows, C, eps);
        return sei_launch_status();
    }
    switch (ln_group(C)) {
        case 1: return launch_ln_fwd<1>(x, gamma, beta, y, mean, rstd, rows, C, eps, s);
        case 2: return launch_ln_fwd<2>(x, gamma, beta, y, mean, rstd, rows, C, eps, s);
        case 4: return launch_ln_fwd<4>(x, gamma, beta, y, mean, rstd, rows, C, eps, s);
        case 8: return launch_ln_fwd<8>(x, gamma, beta, y, mean, rstd, rows, C, eps, s);
        case 16: return launch_ln_fwd<16>(x, gamma, beta, y, mean, rstd, rows, C, eps, s);
        case 32: return launch_ln_fwd<32>(x, gamma, beta, y, mean, rstd, rows, C, eps, s);
        default: return launch_ln_fwd<64>(x, gamma, beta, y, mean, rstd, rows, C, eps, s);
    }
}

namespace {
// launch plan of sei_ln_bwd; workspace = [stats: 2*rows floats (wide only)] [partials: nparts * 2C floats]
struct LnBwdPlan {
    int kind;                 // 0 legacy (atomics, no workspace), 1 narrow vectorised, 2 wide two-pass, 3 wide one-pass
    int G, NV;
    unsigned grid, col_blocks, chunks;
    int rows_per_chunk;
    size_t stats_floats, nparts;
};
inline LnBwdPlan ln_bwd_plan(size_t rows, int C) {
    LnBwdPlan p{};
    if (C % 4 != 0 || C < 8) return p;
    if (C <= 512) {
        const int q = C / 4;                                  // float4 per row
        if ((q & (q - 1)) != 0) return p;                     // power of two only
        p.NV = q > 64 ? q / 64 : 1;
        p.G = q / p.NV;
        p.kind = 1;
        const size_t sweeps = sei_ceil_div(rows, (size_t)(LN_THREADS / p.G));
        size_t cap = ((size_t)1 << 20) / (2 * (size_t)C);     // <= 1M partial floats
        if (cap > 512) cap = 512;                             // two workgroups per CU stream at full rate; fewer partials to fold
        p.grid = (unsigned)(sweeps < cap ? sweeps : cap);
        p.nparts = p.grid;
        return p;
    }
    if (C % 1024 == 0 && C <= 8192 && rows >= 64) {            // whole rows per workgroup, x and gy read once
        p.kind = 3;
        p.NV = C / 1024;
        const size_t cap = C >= 8192 ? 256 : 512;               // partial rows: 2 C floats each (<= 17 MB)
        p.grid = (unsigned)(rows < cap ? rows : cap);
        p.nparts = p.grid;
        return p;
    }
    p.kind = 2;
    p.col_blocks = (unsigned)sei_ceil_div((size_t)C, 4 * LN_THREADS);
    size_t chunks = 768 / p.col_blocks > 0 ? 768 / p.col_blocks : 1;       // ~768 workgroups in pass 2
    if (chunks > rows) chunks = rows;
    p.rows_per_chunk = (int)sei_ceil_div(rows, chunks);
    p.chunks = (unsigned)sei_ceil_div(rows, (size_t)p.rows_per_chunk);
    p.stats_floats = 2 * rows;
    p.nparts = p.chunks;
    return p;
}
}  // namespace

extern "C" size_t sei_ln_bwd_workspace(size_t rows, int C) {
    if (rows == 0 || C <= 0) return 0;
    const LnBwdPlan p = ln_bwd_plan(rows, C);
    return p.stats_floats + p.nparts * 2 * (size_t)C;
}

// Where the partial sums of sei_ln_bwd lie in its workspace ([parts][2 C] floats from this offset on), and how many
// there are (0: this shape adds with atomics and leaves nothing to fold).
extern "C" size_t sei_ln_bwd_part_offset(size_t rows, int C) {
    if (rows == 0 || C <= 0) return 0;
    return ln_bwd_plan(rows, C).stats_floats;
}
extern "C" size_t sei_ln_bwd_part_count(size_t rows, int C) {
    if (rows == 0 || C <= 0) return 0;
    const LnBwdPlan p = ln_bwd_plan(rows, C);
    return p.kind != 0 ? p.nparts : 0;
}

extern "C" int sei_ln_bwd(const float *x, const float *gamma, const float *mean, const float *rstd,
                          const float *gy, float *gx, float *ggamma, float *gbeta, size_t rows, int C,
                          float *work, size_t work_floats, void *stream) {
    return sei_ln_bwd_res(x, gamma, mean, rstd, gy, nullptr, gx, ggamma, gbeta, rows, C, work, work_floats, stream);
}

extern "C" int sei_ln_bwd_res(const float *x, const float *gamma, const float *mean, const float *rstd,
                              const float *gy, const float *res, float *gx, float *ggamma, float *gbeta, size_t rows,
                              int C, float *work, size_t work_floats, void *stream) {
    SEI_REQUIRE(x && gamma && mean && rstd && gy && gx && rows > 0 && C > 0);
    SEI_REQUIRE(!res || sei_ln_bwd_part_count(rows, C) > 0);       // the residual rides in the vectorised kernels only
    // ggamma = gbeta = NULL: the partial sums stay in `work` for sei_fold_many (shapes with sei_ln_bwd_part_count > 0)
    SEI_REQUIRE((ggamma != nullptr) == (gbeta != nullptr));
    SEI_REQUIRE(ggamma || sei_ln_bwd_part_count(rows, C) > 0);
    if (C > LN_WIDE_EPT * LN_THREADS) return SEI_ERR_TOO_LARGE;
    hipStream_t s = (hipStream_t)stream;
    const LnBwdPlan p = ln_bwd_plan(rows, C);
    if (p.kind != 0) {
        SEI_REQUIRE(work && work_floats >= p.stats_floats + p.nparts * 2 * (size_t)C);
        SEI_REQUIRE(rows < ((size_t)1 << 31));
        float *part = work + p.stats_floats;
        if (p.kind == 1) {
#define SEI_LN_VEC(GG, NN)                                                                                    \
    hipLaunchKernelGGL((ln_bwd_vec_kernel<GG, NN>), dim3(p.grid), dim3(LN_THREADS), 0, s, x, gamma, mean, rstd, \
                       gy, res, gx, part, rows);                                                              \
    break;
            switch (p.G * 100 + p.NV) {
                case 201: SEI_LN_VEC(2, 1)
                case 401: SEI_LN_VEC(4, 1)
                case 801: SEI_LN_VEC(8, 1)
                case 1601: SEI_LN_VEC(16, 1)
                case 3201: SEI_LN_VEC(32, 1)
                case 6401: SEI_LN_VEC(64, 1)
                case 6402: SEI_LN_VEC(64, 2)
                default: return SEI_ERR_BAD_ARG;
            }
#undef SEI_LN_VEC
        } else if (p.kind == 3) {
#define SEI_LN_ROW(NN)                                                                                        \
    hipLaunchKernelGGL((ln_bwd_row_kernel<NN>), dim3(p.grid), dim3(LN_THREADS), 0, s, x, gamma, mean, rstd, gy, \
                       res, gx, part, rows);                                                                  \
    break;
            switch (p.NV) {
                case 1: SEI_LN_ROW(1)
                case 2: SEI_LN_ROW(2)
                case 3: SEI_LN_ROW(3)
                case 4: SEI_LN_ROW(4)
                case 5: SEI_LN_ROW(5)
                case 6: SEI_LN_ROW(6)
                case 7: SEI_LN_ROW(7)
                default: SEI_LN_ROW(8)
            }
#undef SEI_LN_ROW
        } else {
            float2 *stats = reinterpret_cast<float2 *>(work);
            hipLaunchKernelGGL(ln_bwd_rowstats_kernel, dim3((unsigned)rows), dim3(LN_THREADS), 0, s, x, gamma, mean,
                               rstd, gy, stats, C);
            hipLaunchKernelGGL(ln_bwd_cols_kernel, dim3(p.col_blocks, p.chunks), dim3(LN_THREADS), 0, s, x, gamma,
                               mean, rstd, gy, (const float2 *)stats, res, gx, part, rows, C, p.rows_per_chunk);
        }
        if (ggamma) return sei_fold_now(sei_fold_job(SEI_FOLD_SPLIT, part, (int)p.nparts, 2 * C, C, ggamma, gbeta, nullptr), s);
        return sei_launch_status();
    }
    // legacy shapes (C not a multiple of 4, or not 4 * 2^k below 512): scalar lanes, float atomics
    if (C > 64 * LN_EPL) {
        hipLaunchKernelGGL(ln_bwd_wide_kernel, dim3(sei_capped_grid(rows, 2, 512)), dim3(LN_THREADS), 0, s, x, gamma,
                           mean, rstd, gy, gx, ggamma, gbeta, rows, C);
        return sei_launch_status();
    }
    switch (ln_group(C)) {
        case 1: return launch_ln_bwd<1>(x, gamma, mean, rstd, gy, gx, ggamma, gbeta, rows, C, s);
        case 2: return launch_ln_bwd<2>(x, gamma, mean, rstd, gy, gx, ggamma, gbeta, rows, C, s);
        case 4: return launch_ln_bwd<4>(x, gamma, mean, rstd, gy, gx, ggamma, gbeta, rows, C, s);
        case 8: return launch_ln_bwd<8>(x, gamma, mean, rstd, gy, gx, ggamma, gbeta, rows, C, s);
        case 16: return launch_ln_bwd<16>(x, gamma, mean, rstd, gy, gx, ggamma, gbeta, rows, C, s);
        case 32: return launch_ln_bwd<32>(x, gamma, mean, rstd, gy, gx, ggamma, gbeta, rows, C, s);
        default: return launch_ln_bwd<64>(x, gamma, mean, rstd, gy, gx, ggamma, gbeta, rows, C, s);
    }
}
