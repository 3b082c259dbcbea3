// The Deep Image Prior decoder (models/dip.py: deepinv v0.2.0's ConvDecoder restated) for gfx950, float32, batch 1,
// 32 channels. Activations are channels-last, [H * W][32]; weights are read in torch's own layout straight from the flat
// parameter bucket ([co][ci][ky][kx] for the 3x3 stages, [o][c] for the 1x1 head). A stage is
//
//     u   = nearest_upsample(BN_{l-1}(a_{l-1}))          never stored: an affine (scale, shift) and an index map on load
//     a_l = relu(conv3x3(u) + bias)                      stored, with its channel statistics
//
// and BN_l is applied by whoever reads a_l (the next stage, or the head). The convolution's zero padding is zero in u's
// domain: a tap outside the image contributes 0, not `shift`.
//
//   dip_stage_fwd_kernel   one pixel x 32 output channels per thread, 256 pixels per workgroup, the 36 KiB weight block
//                          in LDS as [tap][ci][co] (every lane reads the same 16 bytes: a broadcast), inputs through the
//                          index map from global memory (neighbouring pixels share them: L1 / L2 hits), 9216 VALU FMAs
//                          per pixel. Epilogue: per-workgroup (sum, M2 about the workgroup's own mean) of a_l per channel.
//   dip_bn_finalize_kernel Chan's pairwise combination of those partials in double -> mean, rstd, scale, shift.
//   dip_head_fwd_kernel    BN-apply + 1x1 convolution + bias to NCHW.
//   dip_head_bwd_kernel    gradient with respect to the last BN's output, per-workgroup partials of the head's gradients.
//   dip_bn_bwd_*           the two channel sums (g x_norm -> g_gamma, g -> g_beta), then in place
//                          g <- relu_mask * scale * (g - mean(g) - x_norm * mean(g x_norm)): the gradient at the conv output.
//   dip_bwd_data_kernel    one SOURCE pixel x 32 input channels per thread: the nearest map is monotone, so a source pixel
//                          owns a contiguous block of destination rows and columns; it evaluates the transposed
//                          convolution (weights in LDS as [tap][co][ci]) at each of them and sums. A gather, no scatter.
//   dip_wgrad_kernel       8 x 32 pixel tiles; u with its halo (through the forward's load path) and g in LDS; a thread
//                          owns one co, four ci and the nine taps (36 accumulators, + the bias sum); a workgroup walks
//                          tiles grid-stride and stores ONE partial block.
//   dip_reduce_parts_kernel sums per-workgroup partials in a fixed order (double accumulator).
//   dip_adam_kernel        sei_adam_element with the step's scalars read from DEVICE memory, so that a captured iteration
//                          does not freeze the step number (sei_adam_fused takes them as launch arguments).
//
// No atomics; every reduction is two-stage through the caller's workspace in a fixed order: bit-reproducible.
#include "sei_common.h"

namespace {

constexpr int DC = 32;                         // channels
constexpr int PIX = 256;                       // pixels (threads) per workgroup of the per-pixel kernels
constexpr int TPAD = DC + 1;                   // row pitch of the LDS transposition tile
constexpr int WT_H = 8, WT_W = 32, WT_HW = WT_W + 2, WT_HALO = (WT_H + 2) * WT_HW;
constexpr int WG_MAX_BLOCKS = 512;
constexpr int WG_N = 9 * DC * DC + DC;         // one partial block of the weight gradient: weights then biases
constexpr int MAX_COUT = 8;
constexpr int MAX_EXTENT = 16384;              // (float)index is exact, pixel counts fit an int

// torch's nearest index: min(floor(dst * (float(in) / float(out))), in - 1)
__device__ __forceinline__ int dip_src(int d, float scale, int in) {
    const int s = (int)floorf((float)d * scale);
    return s < in - 1 ? s : in - 1;
}

// the first destination index whose source is >= s (the map is monotone); s = in gives out
__device__ __forceinline__ int dip_first_dst(int s, float scale, int in, int out) {
    if (s <= 0) return 0;
    if (s >= in) return out;
    int d = (int)ceilf((float)s / scale);
    d = d < 0 ? 0 : (d > out ? out : d);
    while (d > 0 && dip_src(d - 1, scale, in) >= s) --d;
    while (d < out && dip_src(d, scale, in) < s) ++d;
    return d;
}

// Per-channel sum over the workgroup's 256 rows of the tile T[256][TPAD] (rows >= nvalid skipped); `shift` is subtracted
// and the difference squared when SQUARE. Result for channel c in thread c (threads 0..31). `red` holds 256 floats.
template <bool SQUARE>
__device__ __forceinline__ float dip_tile_colsum(const float *T, float *red, int nvalid, float shift) {
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
    float s = 0.f;
    for (int i = 0; i < 32; ++i) {
        const int p = g * 32 + i;
        if (p < nvalid) {
            const float v = T[p * TPAD + c];
            if (SQUARE) {
                const float d = v - shift;
                s = fmaf(d, d, s);
            } else {
                s += v;
            }
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    float total = 0.f;
    if (threadIdx.x < 32)
        for (int k = 0; k < 8; ++k) total += red[k * 32 + c];
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(PIX) void dip_stage_fwd_kernel(const float *__restrict__ a_prev, const float *__restrict__ ss,
                                                            const float *__restrict__ w, const float *__restrict__ bias,
                                                            float *__restrict__ a_out, float *__restrict__ part, int Hin,
                                                            int Win, int Hout, int Wout, float sy, float sx) {
    __shared__ float Ws[9 * DC * DC];          // [tap][ci][co]; reused as the transposition tile (256 * 33 <= 9216)
    __shared__ float SS[2 * DC];
    __shared__ float red[PIX];
    __shared__ float bmean[DC];
    const int tid = threadIdx.x;
    for (int i = tid; i < 9 * DC * DC; i += PIX) {
        const int co = i / (9 * DC), rem = i - co * 9 * DC, ci = rem / 9, tap = rem - ci * 9;
        Ws[(tap * DC + ci) * DC + co] = w[i];
    }
    if (tid < 2 * DC) SS[tid] = ss ? ss[tid] : (tid < DC ? 1.f : 0.f);
    __syncthreads();

    const int HW = Hout * Wout;
    const int first = blockIdx.x * PIX;
    const int nvalid = HW - first < PIX ? HW - first : PIX;
    const bool valid = tid < nvalid;
    const int p = valid ? first + tid : HW - 1;
    const int y = p / Wout, x = p - y * Wout;

    float acc[DC];
#pragma unroll
    for (int co = 0; co < DC; ++co) acc[co] = bias[co];
    // (the three outer loops stay rolled: unrolled, the compiler hoists the loads of a whole tap and spills)
#pragma unroll 1
    for (int ky = 0; ky < 3; ++ky) {
        const int yy = y + ky - 1;
        const bool iny = yy >= 0 && yy < Hout;
        const int srow = dip_src(iny ? yy : 0, sy, Hin);
#pragma unroll 1
        for (int kx = 0; kx < 3; ++kx) {
            const int xx = x + kx - 1;
            const bool inb = iny && xx >= 0 && xx < Wout;
            const int scol = dip_src(inb ? xx : 0, sx, Win);
            const float4 *src = reinterpret_cast<const float4 *>(a_prev + ((size_t)srow * Win + scol) * DC);
            const float *wt = Ws + (ky * 3 + kx) * DC * DC;
#pragma unroll 1
            for (int c4 = 0; c4 < DC / 4; ++c4) {
                const float4 v = src[c4];
                const float in4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int ci = c4 * 4 + k;
                    const float u = inb ? fmaf(in4[k], SS[ci], SS[DC + ci]) : 0.f;
#pragma unroll
                    for (int o4 = 0; o4 < DC / 4; ++o4) {
                        const float4 wv = *reinterpret_cast<const float4 *>(wt + ci * DC + o4 * 4);
                        acc[o4 * 4 + 0] = fmaf(u, wv.x, acc[o4 * 4 + 0]);
                        acc[o4 * 4 + 1] = fmaf(u, wv.y, acc[o4 * 4 + 1]);
                        acc[o4 * 4 + 2] = fmaf(u, wv.z, acc[o4 * 4 + 2]);
                        acc[o4 * 4 + 3] = fmaf(u, wv.w, acc[o4 * 4 + 3]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int co = 0; co < DC; ++co) acc[co] = fmaxf(acc[co], 0.f);
    if (valid) {
        float4 *dst = reinterpret_cast<float4 *>(a_out + (size_t)p * DC);
#pragma unroll
        for (int o4 = 0; o4 < DC / 4; ++o4) dst[o4] = make_float4(acc[o4 * 4], acc[o4 * 4 + 1], acc[o4 * 4 + 2], acc[o4 * 4 + 3]);
    }
    __syncthreads();                           // every thread is done with the weights: the tile takes their place
    float *T = Ws;
#pragma unroll
    for (int co = 0; co < DC; ++co) T[tid * TPAD + co] = acc[co];
    __syncthreads();
    const float sum = dip_tile_colsum<false>(T, red, nvalid, 0.f);
    if (tid < DC) bmean[tid] = sum / (float)nvalid;
    __syncthreads();
    const float m2 = dip_tile_colsum<true>(T, red, nvalid, bmean[tid & 31]);
    if (tid < DC) {
        part[(size_t)blockIdx.x * 2 * DC + tid] = sum;
        part[(size_t)blockIdx.x * 2 * DC + DC + tid] = m2;
    }
}

// stats: mean[32], rstd[32], scale[32], shift[32]
__global__ __launch_bounds__(64) void dip_bn_finalize_kernel(const float *__restrict__ part, int nblocks, int HW,
                                                             const float *__restrict__ gamma,
                                                             const float *__restrict__ beta, float eps,
                                                             float *__restrict__ stats) {
    const int c = threadIdx.x;
    if (c >= DC) return;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    for (int b = 0; b < nblocks; ++b) {
        const int left = HW - b * PIX;
        const double nb = left < PIX ? left : PIX;
        const double mb = (double)part[(size_t)b * 2 * DC + c] / nb, m2b = part[(size_t)b * 2 * DC + DC + c];
        const double delta = mb - mean, tot = n + nb;
        mean += delta * nb / tot;
        m2 += m2b + delta * delta * n * nb / tot;
        n = tot;
    }
    const float meanf = (float)mean;
    const float rstd = (float)(1.0 / sqrt(m2 / n + (double)eps));
    const float scale = gamma[c] * rstd;
    stats[c] = meanf;
    stats[DC + c] = rstd;
    stats[2 * DC + c] = scale;
    stats[3 * DC + c] = beta[c] - meanf * scale;
}

__global__ __launch_bounds__(PIX) void dip_head_fwd_kernel(const float *__restrict__ a, const float *__restrict__ ss,
                                                           const float *__restrict__ w, const float *__restrict__ bias,
                                                           float *__restrict__ x_hat, int HW, int Cout) {
    __shared__ float Wh[MAX_COUT * DC];
    __shared__ float SS[2 * DC];
    const int tid = threadIdx.x;
    if (tid < Cout * DC) Wh[tid] = w[tid];
    if (tid < 2 * DC) SS[tid] = ss[tid];
    __syncthreads();
    const int p = blockIdx.x * PIX + tid;
    if (p >= HW) return;
    float u[DC];
    const float4 *src = reinterpret_cast<const float4 *>(a + (size_t)p * DC);
#pragma unroll
    for (int c4 = 0; c4 < DC / 4; ++c4) {
        const float4 v = src[c4];
        u[c4 * 4 + 0] = fmaf(v.x, SS[c4 * 4 + 0], SS[DC + c4 * 4 + 0]);
        u[c4 * 4 + 1] = fmaf(v.y, SS[c4 * 4 + 1], SS[DC + c4 * 4 + 1]);
        u[c4 * 4 + 2] = fmaf(v.z, SS[c4 * 4 + 2], SS[DC + c4 * 4 + 2]);
        u[c4 * 4 + 3] = fmaf(v.w, SS[c4 * 4 + 3], SS[DC + c4 * 4 + 3]);
    }
    for (int o = 0; o < Cout; ++o) {
        float s = bias[o];
#pragma unroll
        for (int c = 0; c < DC; ++c) s = fmaf(u[c], Wh[o * DC + c], s);
        x_hat[(size_t)o * HW + p] = s;
    }
}

// g_bn[p][c] = sum_o g_x[o][p] w[o][c]; part[block][o * 32 + c] = sum_p g_x[o][p] u[p][c], part[block][Cout * 32 + o] =
// sum_p g_x[o][p] over the workgroup's pixels
__global__ __launch_bounds__(PIX) void dip_head_bwd_kernel(const float *__restrict__ g_x, const float *__restrict__ a,
                                                           const float *__restrict__ ss, const float *__restrict__ w,
                                                           float *__restrict__ g_bn, float *__restrict__ part, int HW,
                                                           int Cout) {
    __shared__ float T[PIX * TPAD];
    __shared__ float GX[PIX * MAX_COUT];
    __shared__ float Wh[MAX_COUT * DC];
    __shared__ float SS[2 * DC];
    const int tid = threadIdx.x;
    if (tid < Cout * DC) Wh[tid] = w[tid];
    if (tid < 2 * DC) SS[tid] = ss[tid];
    __syncthreads();
    const int p = blockIdx.x * PIX + tid;
    const bool valid = p < HW;
    float gx[MAX_COUT];
#pragma unroll
    for (int o = 0; o < MAX_COUT; ++o) {
        gx[o] = (valid && o < Cout) ? g_x[(size_t)o * HW + p] : 0.f;
        GX[tid * MAX_COUT + o] = gx[o];
    }
    if (valid) {
        const float4 *src = reinterpret_cast<const float4 *>(a + (size_t)p * DC);
        float4 *dst = reinterpret_cast<float4 *>(g_bn + (size_t)p * DC);
#pragma unroll
        for (int c4 = 0; c4 < DC / 4; ++c4) {
            const float4 v = src[c4];
            const float in4[4] = {v.x, v.y, v.z, v.w};
            float out4[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c4 * 4 + k;
                T[tid * TPAD + c] = fmaf(in4[k], SS[c], SS[DC + c]);
                float s = 0.f;
#pragma unroll
                for (int o = 0; o < MAX_COUT; ++o)
                    if (o < Cout) s = fmaf(gx[o], Wh[o * DC + c], s);
                out4[k] = s;
            }
            dst[c4] = make_float4(out4[0], out4[1], out4[2], out4[3]);
        }
    } else {
#pragma unroll
        for (int c = 0; c < DC; ++c) T[tid * TPAD + c] = 0.f;
    }
    __syncthreads();
    const int nout = Cout * DC + Cout;
    for (int e = tid; e < nout; e += PIX) {
        float s = 0.f;
        if (e < Cout * DC) {
            const int o = e >> 5, c = e & 31;
            for (int q = 0; q < PIX; ++q) s = fmaf(GX[q * MAX_COUT + o], T[q * TPAD + c], s);
        } else {
            const int o = e - Cout * DC;
            for (int q = 0; q < PIX; ++q) s += GX[q * MAX_COUT + o];
        }
        part[(size_t)blockIdx.x * nout + e] = s;
    }
}

// part[block][c] = sum_p g[p][c] x_norm[p][c], part[block][32 + c] = sum_p g[p][c]
__global__ __launch_bounds__(PIX) void dip_bn_bwd_reduce_kernel(const float *__restrict__ g, const float *__restrict__ a,
                                                                const float *__restrict__ stats,
                                                                float *__restrict__ part, int HW) {
    __shared__ float T[PIX * TPAD];
    __shared__ float red[PIX];
    __shared__ float ST[2 * DC];
    const int tid = threadIdx.x;
    if (tid < 2 * DC) ST[tid] = stats[tid];                        // mean, rstd
    __syncthreads();
    const int first = blockIdx.x * PIX;
    const int nvalid = HW - first < PIX ? HW - first : PIX;
    const bool valid = tid < nvalid;
    float gv[DC];
    if (valid) {
        const float4 *gs = reinterpret_cast<const float4 *>(g + (size_t)(first + tid) * DC);
        const float4 *as = reinterpret_cast<const float4 *>(a + (size_t)(first + tid) * DC);
#pragma unroll
        for (int c4 = 0; c4 < DC / 4; ++c4) {
            const float4 v = gs[c4], av = as[c4];
            const float g4[4] = {v.x, v.y, v.z, v.w}, a4[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c4 * 4 + k;
                gv[c] = g4[k];
                T[tid * TPAD + c] = g4[k] * ((a4[k] - ST[c]) * ST[DC + c]);
            }
        }
    }
    __syncthreads();
    const float sgx = dip_tile_colsum<false>(T, red, nvalid, 0.f);
    if (valid) {
#pragma unroll
        for (int c = 0; c < DC; ++c) T[tid * TPAD + c] = gv[c];
    }
    __syncthreads();
    const float sg = dip_tile_colsum<false>(T, red, nvalid, 0.f);
    if (tid < DC) {
        part[(size_t)blockIdx.x * 2 * DC + tid] = sgx;
        part[(size_t)blockIdx.x * 2 * DC + DC + tid] = sg;
    }
}

// in place: g <- (a > 0) * scale * (g - mean(g) - x_norm * mean(g x_norm)); sums = {sum g x_norm [32], sum g [32]}
__global__ __launch_bounds__(256) void dip_bn_bwd_apply_kernel(float *__restrict__ g, const float *__restrict__ a,
                                                               const float *__restrict__ stats,
                                                               const float *__restrict__ sums, size_t n, float count) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i & 31);
    const float av = a[i];
    const float xn = (av - stats[c]) * stats[DC + c];
    const float mgx = sums[c] / count, mg = sums[DC + c] / count;
    const float v = stats[2 * DC + c] * ((g[i] - mg) - xn * mgx);
    g[i] = av > 0.f ? v : 0.f;
}

__global__ __launch_bounds__(PIX) void dip_bwd_data_kernel(const float *__restrict__ gc, const float *__restrict__ w,
                                                           float *__restrict__ g_prev, int Hin, int Win, int Hout,
                                                           int Wout, float sy, float sx) {
    __shared__ float Wt[9 * DC * DC];          // [tap][co][ci]
    const int tid = threadIdx.x;
    for (int i = tid; i < 9 * DC * DC; i += PIX) {
        const int co = i / (9 * DC), rem = i - co * 9 * DC, ci = rem / 9, tap = rem - ci * 9;
        Wt[(tap * DC + co) * DC + ci] = w[i];
    }
    __syncthreads();
    const int q = blockIdx.x * PIX + tid;
    if (q >= Hin * Win) return;
    const int qy = q / Win, qx = q - qy * Win;
    const int y0 = dip_first_dst(qy, sy, Hin, Hout), y1 = dip_first_dst(qy + 1, sy, Hin, Hout);
    const int x0 = dip_first_dst(qx, sx, Win, Wout), x1 = dip_first_dst(qx + 1, sx, Win, Wout);
    float acc[DC];
#pragma unroll
    for (int ci = 0; ci < DC; ++ci) acc[ci] = 0.f;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x)
            for (int ky = 0; ky < 3; ++ky) {
                const int yy = y - (ky - 1);
                if (yy < 0 || yy >= Hout) continue;
                for (int kx = 0; kx < 3; ++kx) {
                    const int xx = x - (kx - 1);
                    if (xx < 0 || xx >= Wout) continue;
                    const float4 *src = reinterpret_cast<const float4 *>(gc + ((size_t)yy * Wout + xx) * DC);
                    const float *wt = Wt + (ky * 3 + kx) * DC * DC;
#pragma unroll
                    for (int o4 = 0; o4 < DC / 4; ++o4) {
                        const float4 v = src[o4];
                        const float g4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int co = o4 * 4 + k;
#pragma unroll
                            for (int c4 = 0; c4 < DC / 4; ++c4) {
                                const float4 wv = *reinterpret_cast<const float4 *>(wt + co * DC + c4 * 4);
                                acc[c4 * 4 + 0] = fmaf(g4[k], wv.x, acc[c4 * 4 + 0]);
                                acc[c4 * 4 + 1] = fmaf(g4[k], wv.y, acc[c4 * 4 + 1]);
                                acc[c4 * 4 + 2] = fmaf(g4[k], wv.z, acc[c4 * 4 + 2]);
                                acc[c4 * 4 + 3] = fmaf(g4[k], wv.w, acc[c4 * 4 + 3]);
                            }
                        }
                    }
                }
            }
    float4 *dst = reinterpret_cast<float4 *>(g_prev + (size_t)q * DC);
#pragma unroll
    for (int c4 = 0; c4 < DC / 4; ++c4) dst[c4] = make_float4(acc[c4 * 4], acc[c4 * 4 + 1], acc[c4 * 4 + 2], acc[c4 * 4 + 3]);
}

__global__ __launch_bounds__(256) void dip_wgrad_kernel(const float *__restrict__ gc, const float *__restrict__ a_prev,
                                                        const float *__restrict__ ss, float *__restrict__ part, int Hin,
                                                        int Win, int Hout, int Wout, float sy, float sx, int tiles_x,
                                                        int ntiles) {
    __shared__ float U[WT_HALO * DC];
    __shared__ float G[WT_H * WT_W * DC];
    __shared__ float SS[2 * DC];
    const int tid = threadIdx.x, co = tid >> 3, cq = tid & 7;
    float acc[4][9];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[k][t] = 0.f;
    float bsum = 0.f;
    if (tid < 2 * DC) SS[tid] = ss ? ss[tid] : (tid < DC ? 1.f : 0.f);
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        __syncthreads();                       // the previous tile's reads are done (first pass: SS is visible)
        const int ty0 = (tile / tiles_x) * WT_H, tx0 = (tile % tiles_x) * WT_W;
        for (int i = tid; i < WT_HALO * (DC / 4); i += 256) {
            const int px = i >> 3, c4 = (i & 7) * 4;
            const int r = px / WT_HW, c = px - r * WT_HW;
            const int y = ty0 - 1 + r, x = tx0 - 1 + c;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (y >= 0 && y < Hout && x >= 0 && x < Wout) {
                const size_t s = ((size_t)dip_src(y, sy, Hin) * Win + dip_src(x, sx, Win)) * DC + c4;
                const float4 r4 = *reinterpret_cast<const float4 *>(a_prev + s);
                v.x = fmaf(r4.x, SS[c4 + 0], SS[DC + c4 + 0]);
                v.y = fmaf(r4.y, SS[c4 + 1], SS[DC + c4 + 1]);
                v.z = fmaf(r4.z, SS[c4 + 2], SS[DC + c4 + 2]);
                v.w = fmaf(r4.w, SS[c4 + 3], SS[DC + c4 + 3]);
            }
            *reinterpret_cast<float4 *>(U + px * DC + c4) = v;
        }
        for (int i = tid; i < WT_H * WT_W * (DC / 4); i += 256) {
            const int px = i >> 3, c4 = (i & 7) * 4;
            const int y = ty0 + (px >> 5), x = tx0 + (px & 31);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (y < Hout && x < Wout) v = *reinterpret_cast<const float4 *>(gc + ((size_t)y * Wout + x) * DC + c4);
            *reinterpret_cast<float4 *>(G + px * DC + c4) = v;
        }
        __syncthreads();
        const int rows = Hout - ty0 < WT_H ? Hout - ty0 : WT_H, cols = Wout - tx0 < WT_W ? Wout - tx0 : WT_W;
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) {
                const float gv = G[(r * WT_W + c) * DC + co];
                bsum += gv;
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const float4 u4 = *reinterpret_cast<const float4 *>(U + ((r + ky) * WT_HW + c + kx) * DC + cq * 4);
                        acc[0][ky * 3 + kx] = fmaf(gv, u4.x, acc[0][ky * 3 + kx]);
                        acc[1][ky * 3 + kx] = fmaf(gv, u4.y, acc[1][ky * 3 + kx]);
                        acc[2][ky * 3 + kx] = fmaf(gv, u4.z, acc[2][ky * 3 + kx]);
                        acc[3][ky * 3 + kx] = fmaf(gv, u4.w, acc[3][ky * 3 + kx]);
                    }
            }
    }
    float *out = part + (size_t)blockIdx.x * WG_N;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int t = 0; t < 9; ++t) out[co * 9 * DC + (cq * 4 + k) * 9 + t] = acc[k][t];
    if (cq == 0) out[9 * DC * DC + co] = bsum;
}

// out_a[i] = sum_b part[b][i] for i < na, out_b[i - na] for the nb2 entries behind them
__global__ __launch_bounds__(256) void dip_reduce_parts_kernel(const float *__restrict__ part, int nblocks, int stride,
                                                               int na, float *__restrict__ out_a, int nb2,
                                                               float *__restrict__ out_b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= na + nb2) return;
    double s = 0.0;
    for (int b = 0; b < nblocks; ++b) s += (double)part[(size_t)b * stride + i];
    if (i < na) out_a[i] = (float)s;
    else out_b[i - na] = (float)s;
}

// hyper: {beta1, beta2, eps, weight_decay, lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)} (sei_adam_scalars_to_device)
__global__ __launch_bounds__(256) void dip_adam_kernel(float *__restrict__ p, const float *__restrict__ g,
                                                       float *__restrict__ m, float *__restrict__ v, size_t n,
                                                       const float *__restrict__ hyper) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float mi = m[i], vi = v[i];
    const float pn = sei_adam_element(p[i], g[i], mi, vi, hyper[0], hyper[1], hyper[2], hyper[3], hyper[4], hyper[5]);
    m[i] = mi;
    v[i] = vi;
    p[i] = pn;
}

bool dip_extent_ok(int v) { return v >= 1; }

// 0, or the SEI_ERR_* code for the extents of one stage
int dip_check_extents(int Hin, int Win, int Hout, int Wout, int C) {
    if (!dip_extent_ok(Hin) || !dip_extent_ok(Win) || !dip_extent_ok(Hout) || !dip_extent_ok(Wout) || C != DC)
        return SEI_ERR_BAD_ARG;
    if (Hin > MAX_EXTENT || Win > MAX_EXTENT || Hout > MAX_EXTENT || Wout > MAX_EXTENT) return SEI_ERR_TOO_LARGE;
    return 0;
}

int dip_pixel_blocks(int H, int W) { return (int)sei_ceil_div((size_t)H * (size_t)W, (size_t)PIX); }

int dip_wgrad_blocks(int H, int W, int &tiles_x, int &ntiles) {
    tiles_x = (int)sei_ceil_div((size_t)W, (size_t)WT_W);
    ntiles = tiles_x * (int)sei_ceil_div((size_t)H, (size_t)WT_H);
    return ntiles < WG_MAX_BLOCKS ? ntiles : WG_MAX_BLOCKS;
}

bool dip_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
bool dip_aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace

extern "C" size_t sei_dip_work_floats(int H, int W, int C, int Cout) {
    if (dip_check_extents(1, 1, H, W, C) != 0 || Cout < 1 || Cout > MAX_COUT) return 0;
    int tiles_x, ntiles;
    const size_t nb = (size_t)dip_pixel_blocks(H, W), wg = (size_t)dip_wgrad_blocks(H, W, tiles_x, ntiles);
    size_t need = nb * 2 * DC;
    if (wg * WG_N > need) need = wg * WG_N;
    if (nb * (size_t)(Cout * DC + Cout) > need) need = nb * (size_t)(Cout * DC + Cout);
    return need;
}

extern "C" int sei_dip_stage_fwd(const float *a_prev, const float *ss_prev, const float *w, const float *bias,
                                 const float *gamma, const float *beta, float *a_out, float *stats, int Hin, int Win,
                                 int Hout, int Wout, int C, float eps, float *work, void *stream) {
    SEI_REQUIRE(a_prev && w && bias && gamma && beta && a_out && stats && work);
    const int rc = dip_check_extents(Hin, Win, Hout, Wout, C);
    if (rc != 0) return rc;
    SEI_REQUIRE(eps > 0.f && dip_aligned16(a_prev) && dip_aligned16(a_out) && dip_aligned4(w) && dip_aligned4(bias) &&
                dip_aligned4(gamma) && dip_aligned4(beta) && dip_aligned4(stats) && dip_aligned4(work) &&
                (!ss_prev || dip_aligned4(ss_prev)));
    hipStream_t s = (hipStream_t)stream;
    const int nb = dip_pixel_blocks(Hout, Wout);
    const float sy = (float)Hin / (float)Hout, sx = (float)Win / (float)Wout;
    hipLaunchKernelGGL(dip_stage_fwd_kernel, dim3(nb), dim3(PIX), 0, s, a_prev, ss_prev, w, bias, a_out, work, Hin, Win,
                       Hout, Wout, sy, sx);
    hipLaunchKernelGGL(dip_bn_finalize_kernel, dim3(1), dim3(64), 0, s, (const float *)work, nb, Hout * Wout, gamma, beta,
                       eps, stats);
    return sei_launch_status();
}

extern "C" int sei_dip_head_fwd(const float *a, const float *ss, const float *w, const float *bias, float *x_hat, int H,
                                int W, int C, int Cout, void *stream) {
    SEI_REQUIRE(a && ss && w && bias && x_hat);
    const int rc = dip_check_extents(1, 1, H, W, C);
    if (rc != 0) return rc;
    SEI_REQUIRE(Cout >= 1 && Cout <= MAX_COUT && dip_aligned16(a) && dip_aligned4(ss) && dip_aligned4(w) &&
                dip_aligned4(bias) && dip_aligned4(x_hat));
    hipLaunchKernelGGL(dip_head_fwd_kernel, dim3(dip_pixel_blocks(H, W)), dim3(PIX), 0, (hipStream_t)stream, a, ss, w, bias,
                       x_hat, H * W, Cout);
    return sei_launch_status();
}

extern "C" int sei_dip_head_bwd(const float *g_x, const float *a, const float *ss, const float *w, float *g_bn, float *g_w,
                                float *g_bias, int H, int W, int C, int Cout, float *work, void *stream) {
    SEI_REQUIRE(g_x && a && ss && w && g_bn && g_w && g_bias && work);
    const int rc = dip_check_extents(1, 1, H, W, C);
    if (rc != 0) return rc;
    SEI_REQUIRE(Cout >= 1 && Cout <= MAX_COUT && dip_aligned16(a) && dip_aligned16(g_bn) && dip_aligned4(g_x) &&
                dip_aligned4(ss) && dip_aligned4(w) && dip_aligned4(g_w) && dip_aligned4(g_bias) && dip_aligned4(work));
    hipStream_t s = (hipStream_t)stream;
    const int nb = dip_pixel_blocks(H, W), nout = Cout * DC + Cout;
    hipLaunchKernelGGL(dip_head_bwd_kernel, dim3(nb), dim3(PIX), 0, s, g_x, a, ss, w, g_bn, work, H * W, Cout);
    hipLaunchKernelGGL(dip_reduce_parts_kernel, dim3((unsigned)sei_ceil_div(nout, 256)), dim3(256), 0, s,
                       (const float *)work, nb, nout, Cout * DC, g_w, Cout, g_bias);
    return sei_launch_status();
}

extern "C" int sei_dip_stage_bwd_bn(float *g, const float *a, const float *stats, float *g_gamma, float *g_beta, int H,
                                    int W, int C, float *work, void *stream) {
    SEI_REQUIRE(g && a && stats && g_gamma && g_beta && work);
    const int rc = dip_check_extents(1, 1, H, W, C);
    if (rc != 0) return rc;
    // the apply pass reads both sums through one pointer: g_beta directly behind g_gamma, as in the parameter bucket
    SEI_REQUIRE(g_beta == g_gamma + DC && dip_aligned16(g) && dip_aligned16(a) && dip_aligned4(stats) &&
                dip_aligned4(g_gamma) && dip_aligned4(work));
    hipStream_t s = (hipStream_t)stream;
    const int nb = dip_pixel_blocks(H, W);
    const size_t n = (size_t)H * W * DC;
    hipLaunchKernelGGL(dip_bn_bwd_reduce_kernel, dim3(nb), dim3(PIX), 0, s, (const float *)g, a, stats, work, H * W);
    hipLaunchKernelGGL(dip_reduce_parts_kernel, dim3(1), dim3(256), 0, s, (const float *)work, nb, 2 * DC, DC, g_gamma, DC,
                       g_beta);
    hipLaunchKernelGGL(dip_bn_bwd_apply_kernel, dim3((unsigned)sei_ceil_div(n, 256)), dim3(256), 0, s, g, a, stats,
                       (const float *)g_gamma, n, (float)(H * W));
    return sei_launch_status();
}

extern "C" int sei_dip_stage_bwd_data(const float *g_conv, const float *w, float *g_prev, int Hin, int Win, int Hout,
                                      int Wout, int C, void *stream) {
    SEI_REQUIRE(g_conv && w && g_prev);
    const int rc = dip_check_extents(Hin, Win, Hout, Wout, C);
    if (rc != 0) return rc;
    SEI_REQUIRE(dip_aligned16(g_conv) && dip_aligned16(g_prev) && dip_aligned4(w));
    const float sy = (float)Hin / (float)Hout, sx = (float)Win / (float)Wout;
    hipLaunchKernelGGL(dip_bwd_data_kernel, dim3(dip_pixel_blocks(Hin, Win)), dim3(PIX), 0, (hipStream_t)stream, g_conv, w,
                       g_prev, Hin, Win, Hout, Wout, sy, sx);
    return sei_launch_status();
}

extern "C" int sei_dip_stage_bwd_weight(const float *g_conv, const float *a_prev, const float *ss_prev, float *g_w,
                                        float *g_bias, int Hin, int Win, int Hout, int Wout, int C, float *work,
                                        void *stream) {
    SEI_REQUIRE(g_conv && a_prev && g_w && g_bias && work);
    const int rc = dip_check_extents(Hin, Win, Hout, Wout, C);
    if (rc != 0) return rc;
    SEI_REQUIRE(dip_aligned16(g_conv) && dip_aligned16(a_prev) && dip_aligned4(g_w) && dip_aligned4(g_bias) &&
                dip_aligned4(work) && (!ss_prev || dip_aligned4(ss_prev)));
    hipStream_t s = (hipStream_t)stream;
    int tiles_x, ntiles;
    const int nb = dip_wgrad_blocks(Hout, Wout, tiles_x, ntiles);
    const float sy = (float)Hin / (float)Hout, sx = (float)Win / (float)Wout;
    hipLaunchKernelGGL(dip_wgrad_kernel, dim3(nb), dim3(256), 0, s, g_conv, a_prev, ss_prev, work, Hin, Win, Hout, Wout, sy,
                       sx, tiles_x, ntiles);
    hipLaunchKernelGGL(dip_reduce_parts_kernel, dim3((unsigned)sei_ceil_div(WG_N, 256)), dim3(256), 0, s,
                       (const float *)work, nb, WG_N, 9 * DC * DC, g_w, DC, g_bias);
    return sei_launch_status();
}

extern "C" int sei_dip_adam(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n,
                            const float *hyper6, void *stream) {
    SEI_REQUIRE(param && grad && exp_avg && exp_avg_sq && hyper6 && n > 0);
    SEI_REQUIRE(dip_aligned4(param) && dip_aligned4(grad) && dip_aligned4(exp_avg) && dip_aligned4(exp_avg_sq) &&
                dip_aligned4(hyper6));
    hipLaunchKernelGGL(dip_adam_kernel, dim3((unsigned)sei_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, param,
                       grad, exp_avg, exp_avg_sq, n, hyper6);
    return sei_launch_status();
}
