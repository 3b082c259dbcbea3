// The 3x3 end convolutions of the U-Net for gfx950 (reference: src/models/convolutional.py:174-176), float32.
//
//   sei_conv3x3_fwd / _bwd_weight[_parts] : UNet.in_conv / out_conv, 3x3 'same'
//
// Small parameter gradients are accumulated with float atomics after an in-block LDS reduction (gradients are
// accumulators by contract), or left as partial rows for sei_fold_many (reduce_kernels.hip).
#include "sei_common.h"

namespace {

// =================================================================================================
// 3x3 convolution with small channel counts (in_conv 3->hidden, out_conv hidden->3)
// =================================================================================================
constexpr int C3_THREADS = 256;

__device__ __forceinline__ size_t img_index(int nchw, int b, int c, int i, int j, int C, int H, int W) {
    return nchw ? (((size_t)b * C + c) * H + i) * W + j : (((size_t)b * H + i) * W + j) * C + c;
}

// y[p, co] = bias[co] + sum_{ci,ky,kx} wq(co,ci,ky,kx) * x[p + (ky-1, kx-1), ci]  (+ res[p, co])
// transposed=0: wq = w[co][ci][ky][kx]                    (forward)
// transposed=1: wq = w[ci][co][2-ky][2-kx], w is (Cin_of_fwd=Cout here ... ) i.e. the data gradient:
//               the caller passes Cin = forward Cout and Cout = forward Cin.
__global__ __launch_bounds__(C3_THREADS) void conv3x3_kernel(
    const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias,
    const float *__restrict__ res, float *__restrict__ y, int B, int H, int W, int Cin, int Cout,
    int nchw_in, int nchw_out, int transposed) {
    extern __shared__ __attribute__((aligned(16))) float sw[];   // [ci][tap][co]
    const int nw = Cin * Cout * 9;
    for (int e = threadIdx.x; e < nw; e += C3_THREADS) {
        const int co = e % Cout, t = (e / Cout) % 9, ci = e / (Cout * 9);
        const int ky = t / 3, kx = t % 3;
        sw[e] = transposed ? w[(((size_t)ci * Cout + co) * 3 + (2 - ky)) * 3 + (2 - kx)]
                           : w[(((size_t)co * Cin + ci) * 3 + ky) * 3 + kx];
    }
    __syncthreads();
    const size_t total = (size_t)B * H * W * Cout;
    for (size_t idx = (size_t)blockIdx.x * C3_THREADS + threadIdx.x; idx < total;
         idx += (size_t)gridDim.x * C3_THREADS) {
        // thread order follows the OUTPUT layout so stores coalesce
        int b, i, j, co;
        if (nchw_out) {
            j = (int)(idx % W); i = (int)((idx / W) % H); co = (int)((idx / ((size_t)W * H)) % Cout);
            b = (int)(idx / ((size_t)W * H * Cout));
        } else {
            co = (int)(idx % Cout); j = (int)((idx / Cout) % W); i = (int)((idx / ((size_t)Cout * W)) % H);
            b = (int)(idx / ((size_t)Cout * W * H));
        }
        float a = bias ? bias[co] : 0.f;
        for (int ky = 0; ky < 3; ++ky) {
            const int ii = i + ky - 1;
            if (ii < 0 || ii >= H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int jj = j + kx - 1;
                if (jj < 0 || jj >= W) continue;
                const int t = ky * 3 + kx;
                for (int ci = 0; ci < Cin; ++ci)
                    a = fmaf(sw[(ci * 9 + t) * Cout + co], x[img_index(nchw_in, b, ci, ii, jj, Cin, H, W)], a);
            }
        }
        const size_t o = img_index(nchw_out, b, co, i, j, Cout, H, W);
        if (res) a += res[o];
        y[o] = a;
    }
}

// gw[co][ci][ky][kx] += sum_p gy[p,co] * x[p + (ky-1,kx-1), ci];  gb[co] += sum_p gy[p,co]
// Each thread owns a set of (co,ci,tap) outputs and walks this block's pixel range.
__global__ __launch_bounds__(C3_THREADS) void conv3x3_bwd_weight_kernel(
    const float *__restrict__ x, const float *__restrict__ gy, float *__restrict__ gw,
    float *__restrict__ gb, int B, int H, int W, int Cin, int Cout, int nchw_x, int nchw_gy,
    int pix_per_block) {
    const size_t npix = (size_t)B * H * W;
    const size_t p0 = (size_t)blockIdx.x * pix_per_block;
    const size_t p1 = min(npix, p0 + pix_per_block);
    const int nw = Cin * Cout * 9;
    for (int e = threadIdx.x; e < nw + Cout; e += C3_THREADS) {
        float acc = 0.f;
        if (e < nw) {
            const int kx = e % 3, ky = (e / 3) % 3, ci = (e / 9) % Cin, co = e / (9 * Cin);
            for (size_t p = p0; p < p1; ++p) {
                const int j = (int)(p % W), i = (int)((p / W) % H), b = (int)(p / ((size_t)W * H));
                const int ii = i + ky - 1, jj = j + kx - 1;
                if (ii < 0 || ii >= H || jj < 0 || jj >= W) continue;
                acc = fmaf(gy[img_index(nchw_gy, b, co, i, j, Cout, H, W)],
                           x[img_index(nchw_x, b, ci, ii, jj, Cin, H, W)], acc);
            }
            atomicAdd(gw + e, acc);
        } else if (gb) {
            const int co = e - nw;
            for (size_t p = p0; p < p1; ++p) {
                const int j = (int)(p % W), i = (int)((p / W) % H), b = (int)(p / ((size_t)W * H));
                acc += gy[img_index(nchw_gy, b, co, i, j, Cout, H, W)];
            }
            atomicAdd(gb + co, acc);
        }
    }
}

// Pixel-per-thread form for the two real cases (3 -> hidden and hidden -> 3): one thread owns one output
// pixel and all COUT accumulators; every input value is loaded once and multiplied into the COUT
// accumulators with weights read as LDS broadcasts. Stores follow the output layout.
template <int COUT>
__global__ __launch_bounds__(C3_THREADS) void conv3x3_pix_kernel(
    const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias,
    const float *__restrict__ res, float *__restrict__ y, int B, int H, int W, int Cin, int nchw_in,
    int nchw_out, int transposed) {
    extern __shared__ __attribute__((aligned(16))) float sw[];   // [ci][tap][co]
    const int nw = Cin * COUT * 9;
    for (int e = threadIdx.x; e < nw; e += C3_THREADS) {
        const int co = e % COUT, t = (e / COUT) % 9, ci = e / (COUT * 9);
        const int ky = t / 3, kx = t % 3;
        sw[e] = transposed ? w[(((size_t)ci * COUT + co) * 3 + (2 - ky)) * 3 + (2 - kx)]
                           : w[(((size_t)co * Cin + ci) * 3 + ky) * 3 + kx];
    }
    __syncthreads();
    const size_t npix = (size_t)B * H * W;
    for (size_t p = (size_t)blockIdx.x * C3_THREADS + threadIdx.x; p < npix; p += (size_t)gridDim.x * C3_THREADS) {
        const int j = (int)(p % W), i = (int)((p / W) % H), b = (int)(p / ((size_t)W * H));
        float acc[COUT];
#pragma unroll
        for (int co = 0; co < COUT; ++co) acc[co] = bias ? bias[co] : 0.f;
        for (int ky = 0; ky < 3; ++ky) {
            const int ii = i + ky - 1;
            if (ii < 0 || ii >= H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int jj = j + kx - 1;
                if (jj < 0 || jj >= W) continue;
                const int t = ky * 3 + kx;
                if (nchw_in) {
                    const float *xp = x + ((size_t)b * Cin * H + ii) * W + jj;
                    for (int ci = 0; ci < Cin; ++ci) {
                        const float v = xp[(size_t)ci * H * W];
                        const float *wr = sw + (ci * 9 + t) * COUT;
#pragma unroll
                        for (int co = 0; co < COUT; ++co) acc[co] = fmaf(wr[co], v, acc[co]);
                    }
                } else {
                    const float *xp = x + (((size_t)b * H + ii) * W + jj) * Cin;
                    for (int ci = 0; ci < Cin; ++ci) {
                        const float v = xp[ci];
                        const float *wr = sw + (ci * 9 + t) * COUT;
#pragma unroll
                        for (int co = 0; co < COUT; ++co) acc[co] = fmaf(wr[co], v, acc[co]);
                    }
                }
            }
        }
        if (nchw_out) {
#pragma unroll
            for (int co = 0; co < COUT; ++co) {
                const size_t o = (((size_t)b * COUT + co) * H + i) * W + j;
                y[o] = res ? acc[co] + res[o] : acc[co];
            }
        } else {
            float *yp = y + p * COUT;
            const float *rp = res ? res + p * COUT : nullptr;
#pragma unroll
            for (int co = 0; co < COUT; ++co) yp[co] = rp ? acc[co] + rp[co] : acc[co];
        }
    }
}

// Image (CS <= 4 channels, either layout) -> the 32 hidden channels in NHWC, and (transposed = 1) the data gradient of a
// hidden -> image convolution: FOUR lanes per pixel, eight output channels each. The pixel-per-thread form above stores
// its 32 values as 32 four-byte stores 128 bytes apart from lane to lane (0.06 of the HBM rate, all of it store issue);
// here a pixel's 128 output bytes leave as 4 x 2 sixteen-byte stores of neighbouring lanes, the 9 x CS input values of
// a pixel are loads shared by its four lanes, the weights are LDS reads of [ci][tap][32] rows (two float4 per lane).
template <int CS>
__global__ __launch_bounds__(C3_THREADS) void conv3x3_small_to_c32_kernel(
    const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias,
    const float *__restrict__ res, float *__restrict__ y, int B, int H, int W, int nchw_in, int transposed) {
    __shared__ __attribute__((aligned(16))) float sw[CS * 9 * 32];   // [ci][tap][co]
    for (int e = threadIdx.x; e < CS * 9 * 32; e += C3_THREADS) {
        const int co = e & 31, t = (e >> 5) % 9, ci = e / (32 * 9);
        sw[e] = transposed ? w[((size_t)ci * 32 + co) * 9 + (8 - t)] : w[((size_t)co * CS + ci) * 9 + t];
    }
    __syncthreads();
    const int q = threadIdx.x & 3;
    float4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
    if (bias) {
        b0 = *reinterpret_cast<const float4 *>(bias + 8 * q);
        b1 = *reinterpret_cast<const float4 *>(bias + 8 * q + 4);
    }
    const size_t npix = (size_t)B * H * W;
    for (size_t p = ((size_t)blockIdx.x * C3_THREADS + threadIdx.x) >> 2; p < npix; p += ((size_t)gridDim.x * C3_THREADS) >> 2) {
        const int j = (int)(p % W), i = (int)((p / W) % H), b = (int)(p / ((size_t)W * H));
        float4 a0 = b0, a1 = b1;
        // (round 5: ONE 64-bit pixel address, then 32-bit tap / channel offsets -- img_index() per tap and channel was three
        // 64-bit multiplies each: a PMC pass counted 697 VALU instructions per wave around its 216 FMAs)
        const float *px = x + (nchw_in ? ((size_t)b * CS * H + i) * W + j : (((size_t)b * H + i) * W + j) * CS);
        const int pstr = nchw_in ? 1 : CS, cstr = nchw_in ? H * W : 1;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int ii = i + ky - 1;
            if (ii < 0 || ii >= H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int jj = j + kx - 1;
                if (jj < 0 || jj >= W) continue;
                const float *tp = px + ((ky - 1) * W + (kx - 1)) * pstr;
#pragma unroll
                for (int ci = 0; ci < CS; ++ci) {
                    const float v = tp[ci * cstr];
                    const float4 w0 = *reinterpret_cast<const float4 *>(sw + (ci * 9 + ky * 3 + kx) * 32 + 8 * q);
                    const float4 w1 = *reinterpret_cast<const float4 *>(sw + (ci * 9 + ky * 3 + kx) * 32 + 8 * q + 4);
                    a0.x = fmaf(w0.x, v, a0.x); a0.y = fmaf(w0.y, v, a0.y); a0.z = fmaf(w0.z, v, a0.z); a0.w = fmaf(w0.w, v, a0.w);
                    a1.x = fmaf(w1.x, v, a1.x); a1.y = fmaf(w1.y, v, a1.y); a1.z = fmaf(w1.z, v, a1.z); a1.w = fmaf(w1.w, v, a1.w);
                }
            }
        }
        float *yp = y + p * 32 + 8 * q;
        if (res) {
            const float4 r0 = *reinterpret_cast<const float4 *>(res + p * 32 + 8 * q);
            const float4 r1 = *reinterpret_cast<const float4 *>(res + p * 32 + 8 * q + 4);
            a0.x += r0.x; a0.y += r0.y; a0.z += r0.z; a0.w += r0.w;
            a1.x += r1.x; a1.y += r1.y; a1.z += r1.z; a1.w += r1.w;
        }
        *reinterpret_cast<float4 *>(yp) = a0;
        *reinterpret_cast<float4 *>(yp + 4) = a1;
    }
}

// Weight gradient, tiled: a workgroup stages P pixels of gy (P x Cout) and of the im2col'ed input
// (P x Cin*9) in LDS, each thread owns a few of the Cout*Cin*9 outputs and reduces over the P pixels
// out of LDS; one float atomic per output per workgroup.
__global__ __launch_bounds__(C3_THREADS) void conv3x3_bwd_weight_tiled_kernel(
    const float *__restrict__ x, const float *__restrict__ gy, float *__restrict__ gw,
    float *__restrict__ gb, int B, int H, int W, int Cin, int Cout, int nchw_x, int nchw_gy, int P,
    int tiles_per_block) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int KC = Cin * 9;
    float *sG = sm;                 // [P][Cout]
    float *sX = sm + P * Cout;      // [P][KC]
    const size_t npix = (size_t)B * H * W;
    const int nout = Cout * KC;
    constexpr int MAXO = 8;         // outputs per thread (nout <= 8*256)
    float acc[MAXO];
#pragma unroll
    for (int q = 0; q < MAXO; ++q) acc[q] = 0.f;
    float accb = 0.f;
    for (int tile = 0; tile < tiles_per_block; ++tile) {
        const size_t p0 = ((size_t)blockIdx.x * tiles_per_block + tile) * P;
        if (p0 >= npix) break;
        const int np = (int)min((size_t)P, npix - p0);
        __syncthreads();
        for (int e = threadIdx.x; e < np * Cout; e += C3_THREADS) {
            const int pp = e / Cout, co = e % Cout;
            const size_t p = p0 + pp;
            const int j = (int)(p % W), i = (int)((p / W) % H), b = (int)(p / ((size_t)W * H));
            sG[e] = gy[img_index(nchw_gy, b, co, i, j, Cout, H, W)];
        }
        for (int e = threadIdx.x; e < np * KC; e += C3_THREADS) {
            const int pp = e / KC, k = e % KC;
            const int ci = k / 9, t = k % 9;
            const size_t p = p0 + pp;
            const int j = (int)(p % W), i = (int)((p / W) % H), b = (int)(p / ((size_t)W * H));
            const int ii = i + t / 3 - 1, jj = j + t % 3 - 1;
            sX[e] = (ii >= 0 && ii < H && jj >= 0 && jj < W) ? x[img_index(nchw_x, b, ci, ii, jj, Cin, H, W)] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < MAXO; ++q) {
            const int e = threadIdx.x + q * C3_THREADS;
            if (e < nout) {
                const int co = e / KC, k = e % KC;
                float a = acc[q];
                for (int pp = 0; pp < np; ++pp) a = fmaf(sG[pp * Cout + co], sX[pp * KC + k], a);
                acc[q] = a;
            }
        }
        if (gb && threadIdx.x < Cout)
            for (int pp = 0; pp < np; ++pp) accb += sG[pp * Cout + threadIdx.x];
    }
#pragma unroll
    for (int q = 0; q < MAXO; ++q) {
        const int e = threadIdx.x + q * C3_THREADS;
        if (e < nout) atomicAdd(gw + e, acc[q]);      // e = (co*Cin + ci)*9 + t: the torch weight layout
    }
    if (gb && threadIdx.x < Cout) atomicAdd(gb + threadIdx.x, accb);
}

// -------------------------------------------------------------------------------------------------
// Lane-per-channel forms for the default network (hidden = 32): the 32 lanes of a half-wave are the 32
// hidden channels, so every access to the NHWC hidden tensor is a coalesced 128-byte row (the pixel-per-thread
// kernels above read it with a 128-byte stride ACROSS lanes: 64 cache lines per load). A half-wave walks a
// run of C3L_RUN pixels of one image row with a 3x3 register window sliding by one column per pixel.
// -------------------------------------------------------------------------------------------------
constexpr int C3L_RUN = 16;

__device__ __forceinline__ float half_wave_sum(float v) {        // over the 32 lanes of this half-wave
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// forward hidden(32, NHWC) -> CS <= 4 channels: y[p, co] = bias[co] + sum_{t, ci} w[co][ci][t] x[p + t, ci] (+ res);
// transposed = 1: the data gradient of a CS -> 32 convolution (w is THAT convolution's (32, CS, 3, 3) weight, read with
// flipped taps and swapped channel roles): gx[p, c] = sum_{t, co} w[co][c][8 - t] gy[p + t, co]
template <int CS>
__global__ __launch_bounds__(C3_THREADS) void conv3x3_c32_to_small_kernel(
    const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias,
    const float *__restrict__ res, float *__restrict__ y, int B, int H, int W, int nchw_out, int nruns_row,
    int total_runs, int transposed) {
    const int ci = threadIdx.x & 31, grp = threadIdx.x >> 5;
    float wr[CS][9];
#pragma unroll
    for (int co = 0; co < CS; ++co)
#pragma unroll
        for (int t = 0; t < 9; ++t)
            wr[co][t] = transposed ? w[((size_t)ci * CS + co) * 9 + (8 - t)] : w[((size_t)co * 32 + ci) * 9 + t];
    for (int run = blockIdx.x * (C3_THREADS / 32) + grp; run < total_runs; run += gridDim.x * (C3_THREADS / 32)) {
        const int jr = run % nruns_row, bi = run / nruns_row;
        const int i = bi % H, b = bi / H;
        const int j0 = jr * C3L_RUN, jn = min(C3L_RUN, W - j0);
        const float *xb = x + (size_t)b * H * W * 32 + ci;
        auto load = [&](int ii, int jj) -> float {
            return (ii >= 0 && ii < H && jj >= 0 && jj < W) ? xb[((size_t)ii * W + jj) * 32] : 0.f;
        };
        float win[3][3];                                  // win[ky][slot], slot rotates with the column
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            win[ky][0] = load(i + ky - 1, j0 - 1);
            win[ky][1] = load(i + ky - 1, j0);
        }
        // this lane's (input channel's) share of every output of the run first: part[jl * CS + co]
        float part[C3L_RUN * CS];
#pragma unroll
        for (int jb = 0; jb < C3L_RUN + 2; jb += 3) {
#pragma unroll
            for (int s3 = 0; s3 < 3; ++s3) {
                const int jl = jb + s3;
                if (jl < C3L_RUN) {
                    if (jl < jn) {
#pragma unroll
                        for (int ky = 0; ky < 3; ++ky) win[ky][(s3 + 2) % 3] = load(i + ky - 1, j0 + jl + 1);
                    }
#pragma unroll
                    for (int co = 0; co < CS; ++co) {
                        float a = 0.f;
#pragma unroll
                        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                            for (int kx = 0; kx < 3; ++kx) a = fmaf(wr[co][ky * 3 + kx], win[ky][(s3 + kx) % 3], a);
                        part[jl * CS + co] = a;
                    }
                }
            }
        }
        // ... then ONE transposing butterfly over the 32 lanes for all C3L_RUN * CS sums (round 5): at offset 16, 8, 4, 2 a
        // lane keeps one half of its values and hands the other half to its partner, so the value count halves with the
        // lane distance -- 8 CS + 4 CS + 2 CS + CS exchanges and a last plain stage of CS instead of 5 per sum (240 -> 48 at
        // CS = 3; a PMC pass had 30 of the 45 VALU and all 15 LDS instructions per pixel step in the per-sum butterflies).
        // Every sum is added in the same tree as before: bit-identical. Afterwards lanes 2 jl and 2 jl + 1 both hold the CS
        // outputs of pixel jl.
#define SEI_C3_STAGE(OFF, NV)                                                                   \
        {                                                                                       \
            const bool up = (ci & (OFF)) != 0;                                                  \
            _Pragma("unroll") for (int k = 0; k < (NV) / 2; ++k) {                              \
                const float send = up ? part[k] : part[k + (NV) / 2];                           \
                const float keep = up ? part[k + (NV) / 2] : part[k];                           \
                part[k] = keep + __shfl_xor(send, (OFF), 64);                                   \
            }                                                                                   \
        }
        SEI_C3_STAGE(16, C3L_RUN * CS)
        SEI_C3_STAGE(8, C3L_RUN * CS / 2)
        SEI_C3_STAGE(4, C3L_RUN * CS / 4)
        SEI_C3_STAGE(2, C3L_RUN * CS / 8)
#undef SEI_C3_STAGE
#pragma unroll
        for (int co = 0; co < CS; ++co) part[co] += __shfl_xor(part[co], 1, 64);
        {
            const int jl = ci >> 1;                       // this lane pair's pixel of the run
            if (jl < jn) {
#pragma unroll
                for (int co = 0; co < CS; ++co) {
                    if ((co & 1) != (ci & 1)) continue;   // the pair's two lanes share the CS stores
                    const size_t o = img_index(nchw_out, b, co, i, j0 + jl, CS, H, W);
                    const float v = part[co] + (bias ? bias[co] : 0.f);
                    y[o] = res ? v + res[o] : v;
                }
            }
        }
    }
}

// weight gradient with the 32-channel tensor on the lanes:
//   SMALL_IS_OUT = true : x hidden (NHWC, 32), gy small (CS channels, either layout): gw[co][lane][t], lane = ci
//   SMALL_IS_OUT = false: gy hidden (NHWC, 32), x small (CS channels, either layout): gw[lane][ci][t], lane = co
// Per workgroup: 8 half-wave partials folded through LDS, then one float atomic per output.
template <int CS, bool SMALL_IS_OUT>
__global__ __launch_bounds__(C3_THREADS) void conv3x3_wgrad_c32_kernel(
    const float *__restrict__ x, const float *__restrict__ gy, float *__restrict__ gw, float *__restrict__ gb,
    int B, int H, int W, int nchw_small, int nruns_row, int total_runs) {
    __shared__ float red[C3_THREADS / 32][CS * 9 + CS][32];
    const int lane = threadIdx.x & 31, grp = threadIdx.x >> 5;
    float acc[CS][9];
#pragma unroll
    for (int c = 0; c < CS; ++c)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[c][t] = 0.f;
    float accb[CS];                                      // bias gradient: SMALL_IS_OUT -> per co (lane 0 only);
#pragma unroll                                           //                else -> accb[0] per lane (= co)
    for (int c = 0; c < CS; ++c) accb[c] = 0.f;
    const float *big = SMALL_IS_OUT ? x : gy, *small = SMALL_IS_OUT ? gy : x;
    for (int run = blockIdx.x * (C3_THREADS / 32) + grp; run < total_runs; run += gridDim.x * (C3_THREADS / 32)) {
        const int jr = run % nruns_row, bi = run / nruns_row;
        const int i = bi % H, b = bi / H;
        const int j0 = jr * C3L_RUN, jn = min(C3L_RUN, W - j0);
        if (SMALL_IS_OUT) {
            // window of x (hidden, per lane); gy values of the pixel are uniform over the lanes
            const float *xb = big + (size_t)b * H * W * 32 + lane;
            auto load = [&](int ii, int jj) -> float {
                return (ii >= 0 && ii < H && jj >= 0 && jj < W) ? xb[((size_t)ii * W + jj) * 32] : 0.f;
            };
            float win[3][3];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                win[ky][0] = load(i + ky - 1, j0 - 1);
                win[ky][1] = load(i + ky - 1, j0);
            }
#pragma unroll
            for (int jb = 0; jb < C3L_RUN + 2; jb += 3) {
#pragma unroll
                for (int s3 = 0; s3 < 3; ++s3) {
                    const int jl = jb + s3;
                    if (jl < C3L_RUN && jl < jn) {
#pragma unroll
                        for (int ky = 0; ky < 3; ++ky) win[ky][(s3 + 2) % 3] = load(i + ky - 1, j0 + jl + 1);
#pragma unroll
                        for (int co = 0; co < CS; ++co) {
                            const float g = small[img_index(nchw_small, b, co, i, j0 + jl, CS, H, W)];
                            accb[co] += g;
#pragma unroll
                            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                                for (int kx = 0; kx < 3; ++kx)
                                    acc[co][ky * 3 + kx] = fmaf(g, win[ky][(s3 + kx) % 3], acc[co][ky * 3 + kx]);
                        }
                    }
                }
            }
        } else {
            // gy (hidden, per lane = co) at the pixel; the 3x3xCS window of x is uniform over the lanes
            const float *gb_ = big + ((size_t)(b * H + i) * W) * 32 + lane;
            auto load = [&](int c, int ii, int jj) -> float {
                return (ii >= 0 && ii < H && jj >= 0 && jj < W) ? small[img_index(nchw_small, b, c, ii, jj, CS, H, W)]
                                                                : 0.f;
            };
            float win[CS][3][3];
#pragma unroll
            for (int c = 0; c < CS; ++c)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    win[c][ky][0] = load(c, i + ky - 1, j0 - 1);
                    win[c][ky][1] = load(c, i + ky - 1, j0);
                }
#pragma unroll
            for (int jb = 0; jb < C3L_RUN + 2; jb += 3) {
#pragma unroll
                for (int s3 = 0; s3 < 3; ++s3) {
                    const int jl = jb + s3;
                    if (jl < C3L_RUN && jl < jn) {
#pragma unroll
                        for (int c = 0; c < CS; ++c)
#pragma unroll
                            for (int ky = 0; ky < 3; ++ky) win[c][ky][(s3 + 2) % 3] = load(c, i + ky - 1, j0 + jl + 1);
                        const float g = gb_[(size_t)(j0 + jl) * 32];
                        accb[0] += g;
#pragma unroll
                        for (int c = 0; c < CS; ++c)
#pragma unroll
                            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                                for (int kx = 0; kx < 3; ++kx)
                                    acc[c][ky * 3 + kx] = fmaf(g, win[c][ky][(s3 + kx) % 3], acc[c][ky * 3 + kx]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CS; ++c) {
#pragma unroll
        for (int t = 0; t < 9; ++t) red[grp][c * 9 + t][lane] = acc[c][t];
        red[grp][CS * 9 + c][lane] = accb[c];
    }
    __syncthreads();
    // consecutive threads own consecutive gw addresses (torch layout gw[co][ci][t]): contiguous float atomics --
    // lane-strided ones cost one L2 round per instruction and cache line, serialised over all workgroups
    constexpr int NOUT = CS * 32 * 9;
    for (int o = threadIdx.x; o < NOUT; o += C3_THREADS) {
        const int t = o % 9, rest = o / 9;
        int c, l;                                         // c: the small channel, l: the lane (hidden channel)
        if (SMALL_IS_OUT) {                               // o = (co * 32 + ci) * 9 + t, co = c, ci = l
            l = rest & 31;
            c = rest >> 5;
        } else {                                          // o = (co * CS + ci) * 9 + t, co = l, ci = c
            c = rest % CS;
            l = rest / CS;
        }
        float sum = 0.f;
#pragma unroll
        for (int gI = 0; gI < C3_THREADS / 32; ++gI) sum += red[gI][c * 9 + t][l];
        atomicAdd(gw + o, sum);
    }
    if (gb) {
        const int nb = SMALL_IS_OUT ? CS : 32;
        if ((int)threadIdx.x < nb) {
            float sum = 0.f;
#pragma unroll
            for (int gI = 0; gI < C3_THREADS / 32; ++gI)
                sum += SMALL_IS_OUT ? red[gI][CS * 9 + threadIdx.x][0] : red[gI][CS * 9][threadIdx.x];
            atomicAdd(gb + threadIdx.x, sum);
        }
    }
}

// Weight gradients of the network's two end convolutions on the matrix cores, exact float32 (round 5).
//   hidden tensor BIG (NHWC, 32 channels), small tensor SMALL (CS <= 3 channels, either layout):
//     SMALL_IS_OUT = false (in_conv, x = SMALL, gy = BIG):  gw[co][ci][t] = sum_p BIG[p][co] SMALL[p + off(t)][ci]
//     SMALL_IS_OUT = true  (out_conv, x = BIG, gy = SMALL): gw[co][ci][t] = sum_q BIG[q][ci] SMALL[q - off(t)][co]
//   i.e. one 32 x 32 product  G[m][n] = sum_pixels BIG[pixel][m] P[pixel][n]  with n = (small channel, tap) <= 27 columns of
//   shifted SMALL values (zero outside the image), reduced over all B H W pixels: v_mfma_f32_32x32x2_f32 with two pixels per
//   instruction -- lane (m = lane % 32, k = lane / 32) reads BIG as whole 128-byte pixel rows, lane (n, k) gathers its own
//   shifted SMALL value (a few MB: L2). Column 27 of P is 1 for in_conv: the bias gradient sum_p gy[p][co] falls out of the
//   same product; for out_conv it is the sum of the centre-tap column's values, kept per lane.
// The lane-per-channel kernels above spent 61-68 us per launch (27 FMAs + ~10 loads per pixel and half-wave, 512 workgroups
// adding 864 atomics each onto the same 864 addresses); here a wave owns a contiguous pixel range, a workgroup folds its eight
// accumulator tiles through LDS and 256 workgroups add.
// part != NULL: no atomics -- workgroup g leaves its sums as row g of part ([workgroups][9 * 32 * CS + bias entries], the
// weight gradient in torch's layout followed by the bias gradient) for sei_fold_many (SEI_FOLD_SPLIT, split = 288 CS).
template <bool SMALL_IS_OUT>
__global__ __launch_bounds__(512) void conv3x3_wgrad_mfma_kernel(const float *__restrict__ big, const float *__restrict__ sm,
                                                                 float *__restrict__ gw, float *__restrict__ gb, int B, int H,
                                                                 int W, int CS, int nchw_small, int pix_per_wave,
                                                                 float *__restrict__ part) {
    __shared__ float red[8][1024];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 31, kk = lane >> 5;                    // A: row m = n; B: column n; both: pixel k = kk of the pair
    // this lane's column of P: small channel cn and tap (dy, dx); column 27: ones (in_conv's bias gradient); above: zeros
    const int cn = n / 9, tn = n - 9 * cn;
    const bool col_real = n < 9 * CS, col_ones = !SMALL_IS_OUT && n == 27;
    const int sgn = SMALL_IS_OUT ? -1 : 1;
    const int dy = sgn * (tn / 3 - 1), dx = sgn * (tn % 3 - 1);
    const long long npix = (long long)B * H * W;
    const long long p_begin = ((long long)blockIdx.x * 8 + wave) * pix_per_wave;
    const long long p_end = p_begin + pix_per_wave < npix ? p_begin + pix_per_wave : npix;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float bsum = 0.f;                                            // out_conv: the centre-tap column's running sum
    constexpr int U = 8;                                         // MFMAs (pixel pairs) per batch of loads
    // this lane's pixel (b, i, j): decomposed ONCE, then advanced by two per MFMA (a 64-bit division per pixel and lane made
    // the first version of this kernel VALU-bound: 47 us)
    long long p = p_begin + kk;
    int j = (int)(p % W);
    long long rest = p / W;
    int i = (int)(rest % H), b = (int)(rest / H);
    auto load_batch = [&](float (&av)[U], float (&bv)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool live = p < p_end;
            av[u] = live ? big[(size_t)p * 32 + n] : 0.f;
            const int ii = i + dy, jj = j + dx;
            const bool inside = live && col_real && ii >= 0 && ii < H && jj >= 0 && jj < W;
            const float v = inside ? sm[img_index(nchw_small, b, cn, ii, jj, CS, H, W)] : 0.f;
            bv[u] = (col_ones && live) ? 1.f : v;
            if (SMALL_IS_OUT && tn == 4) bsum += v;              // (dy, dx) = (0, 0): SMALL[q][cn] itself
            p += 2;
            j += 2;
            while (j >= W) {                                     // (W = 1: two rows per step)
                j -= W;
                if (++i == H) {
                    i = 0;
                    ++b;
                }
            }
        }
    };
    auto mfma_batch = [&](const float (&av)[U], const float (&bv)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
    };
    // two batches in registers: the loads of the next 16 pixels are in flight under the MFMAs of these (a wave has ~7
    // batches in all: with load -> wait -> multiply in sequence it spent its time waiting: 32 us per launch)
    float a0[U], b0[U], a1[U], b1[U];
    load_batch(a0, b0);
    for (long long p0 = p_begin; p0 < p_end; p0 += 4 * U) {
        load_batch(a1, b1);                                      // (past the end: all lanes dead, zeros)
        mfma_batch(a0, b0);
        load_batch(a0, b0);
        mfma_batch(a1, b1);
    }
    // accumulator element e of lane (n, kk): G[m = 8 (e / 4) + 4 kk + e % 4][n]
#pragma unroll
    for (int e = 0; e < 16; ++e) red[wave][(8 * (e >> 2) + 4 * kk + (e & 3)) * 32 + n] = acc[e];
    __shared__ float bred[8][64];
    bred[wave][lane] = bsum;
    __syncthreads();
    for (int o = threadIdx.x; o < 1024; o += 512) {
        const int m = o >> 5, nn = o & 31;
        float t = 0.f;
#pragma unroll
        for (int w8 = 0; w8 < 8; ++w8) t += red[w8][o];
        const int nw = 288 * CS;                                 // entries of gw
        float *row = part ? part + (size_t)blockIdx.x * (nw + (SMALL_IS_OUT ? CS : 32)) : nullptr;
        if (nn < 9 * CS) {
            const int c = nn / 9, tap = nn - 9 * c;
            // in_conv: gw[co = m][ci = c][tap]; out_conv: gw[co = c][ci = m][tap]
            const size_t at = SMALL_IS_OUT ? ((size_t)c * 32 + m) * 9 + tap : ((size_t)m * CS + c) * 9 + tap;
            if (row) row[at] = t;
            else atomicAdd(gw + at, t);
        } else if (!SMALL_IS_OUT && nn == 27) {
            if (row) row[nw + m] = t;
            else if (gb) atomicAdd(gb + m, t);
        }
    }
    if (SMALL_IS_OUT && (int)threadIdx.x < CS) {                 // centre-tap lanes: n = 9 c + 4, both pixel halves, all waves
        float t = 0.f;
        const int c = threadIdx.x;
#pragma unroll
        for (int w8 = 0; w8 < 8; ++w8) t += bred[w8][9 * c + 4] + bred[w8][32 + 9 * c + 4];
        if (part) part[(size_t)blockIdx.x * (288 * CS + CS) + 288 * CS + c] = t;
        else if (gb) atomicAdd(gb + c, t);
    }
}

}  // namespace

extern "C" int sei_conv3x3_fwd(const float *x, const float *w, const float *bias, const float *res, float *y,
                               int B, int H, int W, int Cin, int Cout, int nchw_in, int nchw_out,
                               int transposed, void *stream) {
    SEI_REQUIRE(x && w && y && x != y && B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0);
    const size_t lds = sizeof(float) * (size_t)Cin * Cout * 9;
    if (lds > 64 * 1024) return SEI_ERR_TOO_LARGE;
    const size_t npix = (size_t)B * H * W;
    const unsigned pgrid = sei_capped_grid(npix, C3_THREADS, 8192);
    hipStream_t s = (hipStream_t)stream;
    if (Cin == 32 && Cout <= 4 && !nchw_in) {      // hidden -> image (or the data gradient of image -> hidden, whose
        // pixel-per-thread form took 8 ms per launch on the 192 x 192 grids of the x4 network): lanes = hidden channels
        const int nruns_row = (int)sei_ceil_div(W, C3L_RUN);
        const size_t runs = (size_t)B * H * nruns_row;
        SEI_REQUIRE(runs < ((size_t)1 << 31));
        const dim3 grid(sei_capped_grid(runs, C3_THREADS / 32, 65535));
#define SEI_C3_LANES(CS)                                                                                            \
    hipLaunchKernelGGL(conv3x3_c32_to_small_kernel<CS>, grid, dim3(C3_THREADS), 0, s, x, w, bias, res, y, B, H, W, \
                       nchw_out ? 1 : 0, nruns_row, (int)runs, transposed ? 1 : 0);                                 \
    return sei_launch_status();
        switch (Cout) {
            case 1: SEI_C3_LANES(1)
            case 2: SEI_C3_LANES(2)
            case 3: SEI_C3_LANES(3)
            default: SEI_C3_LANES(4)
        }
#undef SEI_C3_LANES
    }
    if (Cout == 32 && Cin <= 4 && !nchw_out && (((uintptr_t)y | (uintptr_t)res | (uintptr_t)bias) & 15) == 0) {
        const unsigned grid4 = sei_capped_grid(npix * 4, C3_THREADS, 16384);
#define SEI_C3_TO32(CS)                                                                                              \
    hipLaunchKernelGGL(conv3x3_small_to_c32_kernel<CS>, dim3(grid4), dim3(C3_THREADS), 0, s, x, w, bias, res, y, B, \
                       H, W, nchw_in ? 1 : 0, transposed ? 1 : 0);                                                  \
    return sei_launch_status();
        switch (Cin) {
            case 1: SEI_C3_TO32(1)
            case 2: SEI_C3_TO32(2)
            case 3: SEI_C3_TO32(3)
            default: SEI_C3_TO32(4)
        }
#undef SEI_C3_TO32
    }
#define SEI_C3_PIX(CO)                                                                                          \
    hipLaunchKernelGGL(conv3x3_pix_kernel<CO>, dim3(pgrid), dim3(C3_THREADS), lds, s, x, w, bias, res, y, B, H, \
                       W, Cin, nchw_in ? 1 : 0, nchw_out ? 1 : 0, transposed ? 1 : 0);                          \
    return sei_launch_status();
    switch (Cout) {
        case 3: SEI_C3_PIX(3)
        case 8: SEI_C3_PIX(8)
        case 16: SEI_C3_PIX(16)
        case 32: SEI_C3_PIX(32)
        default: break;
    }
#undef SEI_C3_PIX
    const size_t total = npix * Cout;
    hipLaunchKernelGGL(conv3x3_kernel, dim3(sei_capped_grid(total, C3_THREADS, 4096)), dim3(C3_THREADS), lds, s, x, w,
                       bias, res, y, B, H, W, Cin, Cout, nchw_in ? 1 : 0, nchw_out ? 1 : 0, transposed ? 1 : 0);
    return sei_launch_status();
}

namespace {
inline bool c3_mfma_ok(size_t npix, int Cin, int Cout, int nchw_x, int nchw_gy) {
    const bool small_out = Cin == 32 && Cout >= 1 && Cout <= 3 && !nchw_x, small_in = Cout == 32 && Cin >= 1 && Cin <= 3 && !nchw_gy;
    return (small_out || small_in) && npix < ((size_t)1 << 40);
}
inline unsigned c3_mfma_grid(size_t npix, size_t workgroups, size_t &ppw) {
    ppw = sei_ceil_div(npix, workgroups * 8);                            // pixels per wave, eight waves per workgroup
    ppw = sei_ceil_div(ppw, 16) * 16;                                   // whole batches of 16 pixels
    return (unsigned)sei_ceil_div(npix, ppw * 8);
}
inline void c3_mfma_launch(const float *x, const float *gy, float *gw, float *gb, float *part, int B, int H, int W, int Cin,
                           int Cout, int nchw_x, int nchw_gy, unsigned grid, size_t ppw, hipStream_t st) {
    if (Cin == 32)
        hipLaunchKernelGGL(conv3x3_wgrad_mfma_kernel<true>, dim3(grid), dim3(512), 0, st, x, gy, gw, gb, B, H, W, Cout,
                           nchw_gy ? 1 : 0, (int)ppw, part);
    else
        hipLaunchKernelGGL(conv3x3_wgrad_mfma_kernel<false>, dim3(grid), dim3(512), 0, st, gy, x, gw, gb, B, H, W, Cin,
                           nchw_x ? 1 : 0, (int)ppw, part);
}
}  // namespace

// Two-stage form of sei_conv3x3_bwd_weight for the network's end convolutions (3 <-> 32 channels): _parts_count = how many
// partial rows the launch leaves (0: shape not served, use sei_conv3x3_bwd_weight), each Cout * Cin * 9 + Cout floats (the
// weight gradient in torch's layout, then the bias gradient); sei_fold_many adds them up (SEI_FOLD_SPLIT, split = Cout * Cin * 9).
// No atomics: 1024 workgroups instead of 256.
extern "C" size_t sei_conv3x3_bwd_weight_parts_count(int B, int H, int W, int Cin, int Cout, int nchw_x, int nchw_gy) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const size_t npix = (size_t)B * H * W;
    if (!c3_mfma_ok(npix, Cin, Cout, nchw_x, nchw_gy)) return 0;
    size_t ppw;
    return c3_mfma_grid(npix, 1024, ppw);
}
extern "C" int sei_conv3x3_bwd_weight_parts(const float *x, const float *gy, float *part, int B, int H, int W, int Cin,
                                            int Cout, int nchw_x, int nchw_gy, void *stream) {
    SEI_REQUIRE(x && gy && part && B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0);
    const size_t npix = (size_t)B * H * W;
    SEI_REQUIRE(c3_mfma_ok(npix, Cin, Cout, nchw_x, nchw_gy));
    size_t ppw;
    const unsigned grid = c3_mfma_grid(npix, 1024, ppw);
    c3_mfma_launch(x, gy, nullptr, nullptr, part, B, H, W, Cin, Cout, nchw_x, nchw_gy, grid, ppw, (hipStream_t)stream);
    return sei_launch_status();
}

extern "C" int sei_conv3x3_bwd_weight(const float *x, const float *gy, float *gw, float *gb, int B, int H,
                                      int W, int Cin, int Cout, int nchw_x, int nchw_gy, void *stream) {
    SEI_REQUIRE(x && gy && gw && B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0);
    const size_t npix = (size_t)B * H * W;
    const int KC = Cin * 9;
    {   // the two real layers of the default network: lanes = the 32 hidden channels
        const bool small_out = Cin == 32 && Cout <= 4 && !nchw_x, small_in = Cout == 32 && Cin <= 4 && !nchw_gy;
        if (c3_mfma_ok(npix, Cin, Cout, nchw_x, nchw_gy)) {
            // (28 columns of the 32 x 32 product: three small channels x nine taps + the bias column)
            size_t ppw;
            const unsigned grid = c3_mfma_grid(npix, 256, ppw);        // one workgroup per CU: 256-way atomics per output
            c3_mfma_launch(x, gy, gw, gb, nullptr, B, H, W, Cin, Cout, nchw_x, nchw_gy, grid, ppw, (hipStream_t)stream);
            return sei_launch_status();
        }
        if (small_out || small_in) {
            const int nruns_row = (int)sei_ceil_div(W, C3L_RUN);
            const size_t runs = (size_t)B * H * nruns_row;
            SEI_REQUIRE(runs < ((size_t)1 << 31));
            // ~512 workgroups: every CU busy, few atomics per output
            const dim3 grid(sei_capped_grid(runs, (C3_THREADS / 32) * (int)sei_ceil_div(runs, (size_t)512 * 8), 65535));
            hipStream_t st = (hipStream_t)stream;
            const int lay = small_out ? (nchw_gy ? 1 : 0) : (nchw_x ? 1 : 0);
#define SEI_C3_WG(CS, OUT)                                                                                          \
    hipLaunchKernelGGL((conv3x3_wgrad_c32_kernel<CS, OUT>), grid, dim3(C3_THREADS), 0, st, x, gy, gw, gb, B, H, W, \
                       lay, nruns_row, (int)runs);                                                                  \
    return sei_launch_status();
            // (the MFMA kernel above owns CS <= 3: only the four-channel small tensor reaches the lane kernel)
            if (small_out) { SEI_C3_WG(4, true) }
            SEI_C3_WG(4, false)
#undef SEI_C3_WG
        }
    }
    if (Cout * KC <= 8 * C3_THREADS) {
        int P = 128;
        while (P > 8 && (size_t)P * (Cout + KC) * sizeof(float) > 48 * 1024) P /= 2;
        int tpb = 1;                          // pixel tiles per workgroup: keep the atomics per output low
        while (sei_ceil_div(npix, (size_t)P * tpb) > 1024) tpb *= 2;
        const size_t lds = (size_t)P * (Cout + KC) * sizeof(float);
        hipLaunchKernelGGL(conv3x3_bwd_weight_tiled_kernel, dim3((unsigned)sei_ceil_div(npix, (size_t)P * tpb)),
                           dim3(C3_THREADS), lds, (hipStream_t)stream, x, gy, gw, gb, B, H, W, Cin, Cout,
                           nchw_x ? 1 : 0, nchw_gy ? 1 : 0, P, tpb);
        return sei_launch_status();
    }
    int ppb = 64;
    while (sei_ceil_div(npix, ppb) > 2048) ppb *= 2;
    hipLaunchKernelGGL(conv3x3_bwd_weight_kernel, dim3((unsigned)sei_ceil_div(npix, ppb)), dim3(C3_THREADS), 0,
                       (hipStream_t)stream, x, gy, gw, gb, B, H, W, Cin, Cout, nchw_x ? 1 : 0, nchw_gy ? 1 : 0,
                       ppb);
    return sei_launch_status();
}
