// Physics operators and the EI scale transform for gfx950 (MI355X).
//
// The blur, the resampler and the scale transform are HBM-streaming stencils on NCHW planar float32 images: each input
// tile (plus halo) is read once from HBM into LDS, both separable passes run out of LDS, the output is written once.
// Algorithmic bytes per plane: 4*H*W in + 4*Ho*Wo out.
//
//   sei_blur_sep_circ / sei_blur_dense_circ : BlurV2.A and its adjoint  (blur/__init__.py:205-227)
//   sei_blur_dense_pad                      : the legacy Blur's replicate / reflect / valid boundaries, both directions
//                                             (blur/__init__.py:34-161), for kernels that are not rank one
//   sei_resample_sepband                    : Downsampling.A, adjoints, AA prefilter; rank-one blurs with those boundaries
//   sei_scale_resample_fwd/bwd              : padded_downsampling_transform (transforms.py:27-83)
//   sei_circ_filter_sep                     : CTLikeFilter.A / A_dagger / filter1d (physics/ct_like_filter.py:10-39)
//
// sei_circ_filter_sep is the dense one of the family: y = C_v x C_h^T with full circulants (every output depends on a
// whole row and a whole column), 2*H*W*(H+W) flop per plane on the float32 vector units against the same 8*H*W bytes.
// One launch, one workgroup per (plane, strip of 32 output columns): the row pass result lives in LDS until the column
// pass has consumed it (see circ_filter_sep_kernel).
#include "sei_common.h"
#include "bicubic_taps.h"
#include "blur_pad.h"

#include <atomic>

namespace {

constexpr int BLUR_THREADS = 256;
constexpr int MAX_TAPS = 63;

// ------------------------------------------------------------------------------------------------
// circular separable blur. One workgroup = one (plane, tile). LDS: taps | input tile + halo | row pass.
// y[i,j] = sum_a tv[a] sum_b th[b] x[(i - a + sv) mod H, (j - b + sh) mod W]
// (the adjoint is the same kernel with flipped taps and sv' = kv-1-sv, done on the host side of the ABI)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLUR_THREADS) void blur_sep_circ_kernel(
    const float *__restrict__ x, float *__restrict__ y, const float *__restrict__ tv,
    const float *__restrict__ th, int kv, int kh, int sv, int sh, int flip, int H, int W, int tile_h,
    int tile_w, int tiles_y, int tiles_x) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int tiles = tiles_y * tiles_x;
    const int plane = blockIdx.x / tiles;
    const int t = blockIdx.x - plane * tiles;
    const int i0 = (t / tiles_x) * tile_h, j0 = (t % tiles_x) * tile_w;
    const int ih = tile_h + kv - 1, iw = tile_w + kh - 1;

    float *s_tv = smem;              // 64 floats reserved each, keeps the tiles 16-byte aligned
    float *s_th = smem + 64;
    float *s_in = smem + 128;
    float *s_row = s_in + ((ih * iw + 3) & ~3);

    if (tid < kv) s_tv[tid] = tv[flip ? kv - 1 - tid : tid];
    if (tid < kh) s_th[tid] = th[flip ? kh - 1 - tid : tid];

    const float *xp = x + (size_t)plane * H * W;
    const int r0 = i0 - kv + 1 + sv, c0 = j0 - kh + 1 + sh;
    for (int idx = tid; idx < ih * iw; idx += BLUR_THREADS) {
        const int r = idx / iw, l = idx - r * iw;
        s_in[idx] = xp[(size_t)sei_mod(r0 + r, H) * W + sei_mod(c0 + l, W)];
    }
    __syncthreads();
    for (int idx = tid; idx < ih * tile_w; idx += BLUR_THREADS) {
        const int r = idx / tile_w, c = idx - r * tile_w;
        const float *src = s_in + r * iw + c + kh - 1;
        float acc = 0.f;
        for (int b = 0; b < kh; ++b) acc = fmaf(s_th[b], src[-b], acc);
        s_row[idx] = acc;
    }
    __syncthreads();
    float *yp = y + (size_t)plane * H * W;
    for (int idx = tid; idx < tile_h * tile_w; idx += BLUR_THREADS) {
        const int r = idx / tile_w, c = idx - r * tile_w;
        if (i0 + r < H && j0 + c < W) {
            const float *src = s_row + (r + kv - 1) * tile_w + c;
            float acc = 0.f;
            for (int a = 0; a < kv; ++a) acc = fmaf(s_tv[a], src[-a * tile_w], acc);
            yp[(size_t)(i0 + r) * W + j0 + c] = acc;
        }
    }
}

// dense (non-separable) circular blur: same tiling, one pass of kv*kh taps out of LDS.
__global__ __launch_bounds__(BLUR_THREADS) void blur_dense_circ_kernel(
    const float *__restrict__ x, float *__restrict__ y, const float *__restrict__ k, int kv, int kh,
    int sv, int sh, int flip, int H, int W, int tile_h, int tile_w, int tiles_y, int tiles_x) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int tiles = tiles_y * tiles_x;
    const int plane = blockIdx.x / tiles;
    const int t = blockIdx.x - plane * tiles;
    const int i0 = (t / tiles_x) * tile_h, j0 = (t % tiles_x) * tile_w;
    const int ih = tile_h + kv - 1, iw = tile_w + kh - 1;
    const int nk = kv * kh;
    float *s_k = smem;
    float *s_in = smem + ((nk + 3) & ~3);
    for (int idx = tid; idx < nk; idx += BLUR_THREADS) s_k[idx] = k[flip ? nk - 1 - idx : idx];
    const float *xp = x + (size_t)plane * H * W;
    const int r0 = i0 - kv + 1 + sv, c0 = j0 - kh + 1 + sh;
    for (int idx = tid; idx < ih * iw; idx += BLUR_THREADS) {
        const int r = idx / iw, l = idx - r * iw;
        s_in[idx] = xp[(size_t)sei_mod(r0 + r, H) * W + sei_mod(c0 + l, W)];
    }
    __syncthreads();
    float *yp = y + (size_t)plane * H * W;
    for (int idx = tid; idx < tile_h * tile_w; idx += BLUR_THREADS) {
        const int r = idx / tile_w, c = idx - r * tile_w;
        if (i0 + r < H && j0 + c < W) {
            float acc = 0.f;
            for (int a = 0; a < kv; ++a) {
                const float *src = s_in + (r + kv - 1 - a) * iw + c + kh - 1;
                for (int b = 0; b < kh; ++b) acc = fmaf(s_k[a * kh + b], src[-b], acc);
            }
            yp[(size_t)(i0 + r) * W + j0 + c] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// dense blur with a replicate / reflect / valid boundary (reference Blur: conv / conv_transpose,
// src/physics/blur/__init__.py:34-161). The tiling of blur_dense_circ_kernel with the staging index map as a template
// parameter and separate input and output extents:
//   y[i,j] = sum_{a,b} k'[a,b] in[map(i - a + Sv), map(j - b + Sh)],   i < Ho, j < Wo,   k' = k or k flipped
// PAD_ZERO reads 0 outside the input: the zero-boundary correlation Z of the adjoint (flipped taps, the output the input
// extended by the padding on every side). Each tap row is summed on its own and the rows are then added in order: a
// fixed order, and the rounding error of kh + kv additions instead of kv * kh.
// ------------------------------------------------------------------------------------------------
// (the staging maps, pad_fetch, are in blur_pad.h: blur_decimate.hip stages through them too)
template <int MODE>
__global__ __launch_bounds__(BLUR_THREADS) void blur_dense_pad_kernel(
    const float *__restrict__ x, float *__restrict__ y, const float *__restrict__ k, int kv, int kh,
    int sv, int sh, int flip, int Hi, int Wi, int Ho, int Wo, int tile_h, int tile_w, int tiles_y, int tiles_x) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int tiles = tiles_y * tiles_x;
    const int plane = blockIdx.x / tiles;
    const int t = blockIdx.x - plane * tiles;
    const int i0 = (t / tiles_x) * tile_h, j0 = (t % tiles_x) * tile_w;
    const int ih = tile_h + kv - 1, iw = tile_w + kh - 1;
    const int nk = kv * kh;
    float *s_k = smem;
    float *s_in = smem + ((nk + 3) & ~3);
    for (int idx = tid; idx < nk; idx += BLUR_THREADS) s_k[idx] = k[flip ? nk - 1 - idx : idx];
    const float *xp = x + (size_t)plane * Hi * Wi;
    const int r0 = i0 - kv + 1 + sv, c0 = j0 - kh + 1 + sh;
    for (int idx = tid; idx < ih * iw; idx += BLUR_THREADS) {
        const int r = idx / iw, l = idx - r * iw;
        s_in[idx] = pad_fetch<MODE>(xp, r0 + r, c0 + l, Hi, Wi);
    }
    __syncthreads();
    float *yp = y + (size_t)plane * Ho * Wo;
    for (int idx = tid; idx < tile_h * tile_w; idx += BLUR_THREADS) {
        const int r = idx / tile_w, c = idx - r * tile_w;
        if (i0 + r < Ho && j0 + c < Wo) {
            float acc = 0.f;
            for (int a = 0; a < kv; ++a) {
                const float *src = s_in + (r + kv - 1 - a) * iw + c + kh - 1;
                float row = 0.f;
                for (int b = 0; b < kh; ++b) row = fmaf(s_k[a * kh + b], src[-b], row);
                acc += row;
            }
            yp[(size_t)(i0 + r) * Wo + j0 + c] = acc;
        }
    }
}

// The adjoint's fold: out[u,v] = sum of Z over the positions (e,f) of the extended canvas, e in [-pv, H-1+pv],
// f in [-ph, W-1+ph], that the axis maps send to (u,v). One thread per output, a gather in a fixed order (rows outer,
// columns inner; reflect: the pixel itself, its mirror about 0, its mirror about n-1): no atomics.
__device__ __forceinline__ int reflect_preimages(int u, int n, int p, int e[3]) {
    int m = 0;
    e[m++] = u;
    if (u >= 1 && u <= p) e[m++] = -u;
    if (u < n - 1 && n - 1 - u <= p) e[m++] = 2 * (n - 1) - u;
    return m;
}

template <int MODE>
__global__ __launch_bounds__(256) void blur_pad_fold_kernel(const float *__restrict__ Z, float *__restrict__ out, int H,
                                                            int W, int pv, int ph, size_t total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int v = (int)(idx % W);
    const size_t q = idx / W;
    const int u = (int)(q % H);
    const size_t plane = q / H;
    const int Wz = W + 2 * ph;
    const float *zp = Z + plane * (size_t)(H + 2 * pv) * Wz;
    float acc = 0.f;
    if (MODE == PAD_REPLICATE) {
        const int e0 = u == 0 ? -pv : u, e1 = u == H - 1 ? H - 1 + pv : u;
        const int f0 = v == 0 ? -ph : v, f1 = v == W - 1 ? W - 1 + ph : v;
        for (int e = e0; e <= e1; ++e) {
            const float *zr = zp + (size_t)(e + pv) * Wz + ph;
            for (int f = f0; f <= f1; ++f) acc += zr[f];
        }
    } else {
        int ev[3], fv[3];
        const int ne = reflect_preimages(u, H, pv, ev), nf = reflect_preimages(v, W, ph, fv);
        for (int a = 0; a < ne; ++a) {
            const float *zr = zp + (size_t)(ev[a] + pv) * Wz + ph;
            for (int b = 0; b < nf; ++b) acc += zr[fv[b]];
        }
    }
    out[idx] = acc;
}

// ------------------------------------------------------------------------------------------------
// separable banded resampling: y = Wv x Wh^T with band-stored weights.
// One workgroup = one (plane, output tile): stage the input footprint, horizontal pass, vertical pass.
// ------------------------------------------------------------------------------------------------
constexpr int RS_THREADS = 256;

__global__ __launch_bounds__(RS_THREADS) void resample_sepband_kernel(
    const float *__restrict__ x, float *__restrict__ y, int Hi, int Wi, int Ho, int Wo,
    const float *__restrict__ wv, const int *__restrict__ lov, int nbv, const float *__restrict__ wh,
    const int *__restrict__ loh, int nbh, int tile_h, int tile_w, int tiles_y, int tiles_x, int fh_max,
    int fw_max) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int tiles = tiles_y * tiles_x;
    const int plane = blockIdx.x / tiles;
    const int t = blockIdx.x - plane * tiles;
    const int oi0 = (t / tiles_x) * tile_h, oj0 = (t % tiles_x) * tile_w;
    const int th = min(tile_h, Ho - oi0), tw = min(tile_w, Wo - oj0);
    const int r0 = lov[oi0], c0 = loh[oj0];
    // input footprint of this tile (clipped to the LDS the host sized from the band-step bound)
    const int fh = min(min(lov[oi0 + th - 1] + nbv, Hi) - r0, fh_max);
    const int fw = min(min(loh[oj0 + tw - 1] + nbh, Wi) - c0, fw_max);
    float *s_in = smem;                              // fh_max * fw_max
    float *s_row = smem + ((fh_max * fw_max + 3) & ~3);   // fh_max * tile_w
    const float *xp = x + (size_t)plane * Hi * Wi;
    for (int idx = tid; idx < fh * fw; idx += RS_THREADS) {
        const int r = idx / fw, c = idx - r * fw;
        s_in[r * fw_max + c] = xp[(size_t)(r0 + r) * Wi + c0 + c];
    }
    __syncthreads();
    for (int idx = tid; idx < fh * tw; idx += RS_THREADS) {
        const int r = idx / tw, c = idx - r * tw;
        const int oj = oj0 + c;
        const int base = loh[oj] - c0;
        const int n = min(nbh, fw - base);
        const float *wrow = wh + (size_t)oj * nbh;
        const float *src = s_in + r * fw_max + base;
        float acc = 0.f;
        for (int b = 0; b < n; ++b) acc = fmaf(wrow[b], src[b], acc);
        s_row[r * tile_w + c] = acc;
    }
    __syncthreads();
    float *yp = y + (size_t)plane * Ho * Wo;
    for (int idx = tid; idx < th * tw; idx += RS_THREADS) {
        const int r = idx / tw, c = idx - r * tw;
        const int oi = oi0 + r;
        const int base = lov[oi] - r0;
        const int n = min(nbv, fh - base);
        const float *wcol = wv + (size_t)oi * nbv;
        float acc = 0.f;
        for (int a = 0; a < n; ++a) acc = fmaf(wcol[a], s_row[(base + a) * tile_w + c], acc);
        yp[(size_t)oi * Wo + oj0 + c] = acc;
    }
}

// ------------------------------------------------------------------------------------------------
// EI scale transform: fused grid generation + bicubic (A=-0.75) gather with reflection.
// The coordinate arithmetic follows the reference's float32 op order (transforms.py:32-41, then
// ATen's grid_sampler unnormalize with align_corners=True), with contraction to FMA disabled
// (__f*_rn intrinsics) so that the sampling positions agree with torch to the last bit wherever
// the division and reciprocal are correctly rounded.
// ------------------------------------------------------------------------------------------------
// (H, W): output / grid size; (Hi, Wi): size of the sampled image (they differ only for the
// antialiased variant, where the reference samples the pre-shrunk image on the original-size grid)
__device__ __forceinline__ void scale_taps(int p, int H, int W, int Hi, int Wi, float two_over_h,
                                           float two_over_w, float inv_rate, float cx, float cy,
                                           ScaleTaps &tp) {
    // position of output pixel p = i*W + j inside the reference's (w,h) meshgrid viewed as (h,w)
    const int aa = p / H, bb = p - aa * H;
    const float v = __fsub_rn(__fmul_rn(two_over_h, (float)bb), 1.f);
    const float u = __fsub_rn(__fmul_rn(two_over_w, (float)aa), 1.f);
    const float gx = __fadd_rn(__fmul_rn(inv_rate, __fsub_rn(v, cx)), cx);
    const float gy = __fadd_rn(__fmul_rn(inv_rate, __fsub_rn(u, cy)), cy);
    bicubic_taps(gx, gy, Hi, Wi, tp);       // bicubic_taps.h
}

__global__ __launch_bounds__(256) void scale_resample_fwd_kernel(
    const float *__restrict__ x, float *__restrict__ y, const float *__restrict__ rate,
    const float *__restrict__ center, int B, int C, int Hi, int Wi, int H, int W, float two_over_h,
    float two_over_w) {
    const size_t total = (size_t)B * H * W;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int b = (int)(idx / ((size_t)H * W));
    const int p = (int)(idx - (size_t)b * H * W);
    ScaleTaps tp;
    scale_taps(p, H, W, Hi, Wi, two_over_h, two_over_w, __fdiv_rn(1.f, rate[b]), center[2 * b],
               center[2 * b + 1], tp);
    for (int c = 0; c < C; ++c) {
        const float *xp = x + ((size_t)b * C + c) * Hi * Wi;
        float acc = 0.f;
#pragma unroll
        for (int dy = 0; dy < 4; ++dy) {
            const float *row = xp + (size_t)tp.ys[dy] * Wi;
            float r = tp.wx[0] * row[tp.xs[0]];
            r = fmaf(tp.wx[1], row[tp.xs[1]], r);
            r = fmaf(tp.wx[2], row[tp.xs[2]], r);
            r = fmaf(tp.wx[3], row[tp.xs[3]], r);
            acc = fmaf(tp.wy[dy], r, acc);
        }
        y[((size_t)b * C + c) * H * W + p] = acc;
    }
}

__global__ __launch_bounds__(256) void scale_resample_bwd_kernel(
    const float *__restrict__ gy, float *__restrict__ gx, const float *__restrict__ rate,
    const float *__restrict__ center, int B, int C, int Hi, int Wi, int H, int W, float two_over_h,
    float two_over_w) {
    const size_t total = (size_t)B * H * W;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int b = (int)(idx / ((size_t)H * W));
    const int p = (int)(idx - (size_t)b * H * W);
    ScaleTaps tp;
    scale_taps(p, H, W, Hi, Wi, two_over_h, two_over_w, __fdiv_rn(1.f, rate[b]), center[2 * b],
               center[2 * b + 1], tp);
    for (int c = 0; c < C; ++c) {
        const float g = gy[((size_t)b * C + c) * H * W + p];
        float *gp = gx + ((size_t)b * C + c) * Hi * Wi;
#pragma unroll
        for (int dy = 0; dy < 4; ++dy)
#pragma unroll
            for (int dx = 0; dx < 4; ++dx)
                atomicAdd(gp + (size_t)tp.ys[dy] * Wi + tp.xs[dx], g * tp.wy[dy] * tp.wx[dx]);
    }
}

// ---- nearest-neighbour rotation about the image centre (deepinv.transform.Rotate -> torchvision rotate) ------------
// Source pixel of output (i, j), in the arithmetic of torchvision's tensor path: base grid xg = j + 0.5 - W/2,
// yg = i + 0.5 - H/2 (its linspace is exact: half-integers), theta rows divided by (W/2, H/2), the three-term product of
// the bmm, then grid_sample's un-normalisation ((g + 1) * size - 1) / 2 and nearbyint (ties to even); out-of-range
// sources read as zero.  All float32, unfused (the file is built with -ffp-contract=off).
struct RotateMap {
    float r00, r10, r01, r11;   // theta[0][0] / (W/2), theta[0][1] / (W/2), theta[1][0] / (H/2), theta[1][1] / (H/2)
};

__device__ __forceinline__ int rotate_source(int p, int H, int W, const RotateMap &m) {
    const int i = p / W, j = p - i * W;
    const float xg = ((float)j + 0.5f) - 0.5f * (float)W, yg = ((float)i + 0.5f) - 0.5f * (float)H;
    const float gx = xg * m.r00 + yg * m.r10, gy = xg * m.r01 + yg * m.r11;
    const float ix = ((gx + 1.f) * (float)W - 1.f) * 0.5f, iy = ((gy + 1.f) * (float)H - 1.f) * 0.5f;
    const float nx = nearbyintf(ix), ny = nearbyintf(iy);
    if (!(nx >= 0.f && nx <= (float)(W - 1) && ny >= 0.f && ny <= (float)(H - 1))) return -1;
    return (int)ny * W + (int)nx;
}

__global__ __launch_bounds__(256) void rotate_nearest_fwd_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                                 int planes, int H, int W, RotateMap m) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= H * W) return;
    const int src = rotate_source(p, H, W, m);
    for (int c = blockIdx.y; c < planes; c += gridDim.y)
        y[(size_t)c * H * W + p] = src < 0 ? 0.f : x[(size_t)c * H * W + src];
}

__global__ __launch_bounds__(256) void rotate_nearest_bwd_kernel(const float *__restrict__ gy, float *__restrict__ gx,
                                                                 int planes, int H, int W, RotateMap m) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= H * W) return;
    const int src = rotate_source(p, H, W, m);
    if (src < 0) return;
    for (int c = blockIdx.y; c < planes; c += gridDim.y)      // several outputs may share a source pixel
        atomicAdd(gx + (size_t)c * H * W + src, gy[(size_t)c * H * W + p]);
}

// ------------------------------------------------------------------------------------------------
// separable dense circular filter: y = C_v x C_h^T, C[i][j] = c[(i - j) mod n] given by its first column.
// One workgroup = one (plane, strip of CF_STRIP output columns, full height). LDS, in floats:
//   s_th  [round_up(W, 32) + W4]   horizontal taps, periodic: s_th[m] = ch[(m - W4) mod W]     (W4 = round_up(W, 4))
//   s_tv  [round_up(H, 8) + H4]    vertical taps,   periodic: s_tv[m] = cv[(m - H4) mod H]
//   s_x   [CF_ROWS][xs]            a chunk of CF_ROWS whole rows of x, zero-padded to W4 columns
//   s_t   [CF_STRIP][ts]           the row pass result, TRANSPOSED (strip column major), zero-padded to H4 rows
// so that both passes are the same inner product of a zero-padded LDS row with a sliding window of taps (cf_dot), with
// no modulo in the loop. Row strides xs / ts are n4 + 4 or n4 + 8, whichever is 4 * odd: eight lanes reading one float4
// each from eight consecutive rows then touch eight different groups of four banks.
// Row pass: thread = (row of the chunk, 4 strip columns); the 32 lanes of a half-wave share their taps (broadcast) and
// read 32 different rows. Column pass: thread = (strip column, 8 output rows); lanes run along the strip, so the
// global stores are 128-byte segments. x is read from global once per strip (the plane stays in L2 after the first).
// ------------------------------------------------------------------------------------------------
constexpr int CF_THREADS = 256;
constexpr int CF_STRIP = 32;
constexpr int CF_ROWS = 32;

__host__ __device__ inline int cf_stride(int n4) { return n4 + (((n4 >> 2) & 1) ? 8 : 4); }

// out[k] = sum_{j < n4} src[j] * taps[tb + k - j], k < NO. src and taps 16-byte aligned, n4 and tb multiples of 4,
// tb >= n4. Each output keeps four partial sums (j mod 4), folded pairwise at the end: every FMA of a step of four
// inputs lands in its own accumulator (no dependent chain inside a step), and the rounding error grows with n / 4.
template <int NO>
__device__ __forceinline__ void cf_dot(const float *__restrict__ src, int n4, const float *__restrict__ taps, int tb,
                                       float (&out)[NO]) {
    float acc[NO][4];
    float w[NO + 4];                    // w[m] = taps[tb - jb - 4 + m]
#pragma unroll
    for (int k = 0; k < NO; ++k) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.f;
#pragma unroll
    for (int q = 0; q < NO / 4; ++q) {
        const float4 t = *reinterpret_cast<const float4 *>(taps + tb + 4 * q);
        w[4 + 4 * q] = t.x; w[5 + 4 * q] = t.y; w[6 + 4 * q] = t.z; w[7 + 4 * q] = t.w;
    }
#pragma unroll 4
    for (int jb = 0; jb < n4; jb += 4) {
        const float4 lo = *reinterpret_cast<const float4 *>(taps + tb - jb - 4);
        const float4 xv = *reinterpret_cast<const float4 *>(src + jb);
        w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w;
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int k = 0; k < NO; ++k) acc[k][jj] = fmaf(xs[jj], w[4 + k - jj], acc[k][jj]);
#pragma unroll
        for (int m = NO + 3; m >= 4; --m) w[m] = w[m - 4];
    }
#pragma unroll
    for (int k = 0; k < NO; ++k) out[k] = (acc[k][0] + acc[k][1]) + (acc[k][2] + acc[k][3]);
}

__global__ __launch_bounds__(CF_THREADS) void circ_filter_sep_kernel(
    const float *__restrict__ x, float *__restrict__ y, const float *__restrict__ cv, const float *__restrict__ ch,
    int H, int W, int strips) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int plane = blockIdx.x / strips;
    const int c0 = (blockIdx.x - plane * strips) * CF_STRIP;
    const int H4 = (H + 3) & ~3, W4 = (W + 3) & ~3;
    const int len_h = ((W + CF_STRIP - 1) & ~(CF_STRIP - 1)) + W4, len_v = ((H + 7) & ~7) + H4;
    const int xs = cf_stride(W4), ts = cf_stride(H4);
    float *s_th = smem;
    float *s_tv = s_th + len_h;
    float *s_x = s_tv + len_v;
    float *s_t = s_x + CF_ROWS * xs;

    for (int m = tid; m < len_h; m += CF_THREADS) s_th[m] = ch[sei_mod(m - W4, W)];
    for (int m = tid; m < len_v; m += CF_THREADS) s_tv[m] = cv[sei_mod(m - H4, H)];

    // row pass: s_t[c][i] = sum_j x[i][j] * ch[(c0 + c - j) mod W], a chunk of CF_ROWS rows at a time
    const float *xp = x + (size_t)plane * H * W;
    const int rr = tid & 31, cq = 4 * (tid >> 5);
    for (int r0 = 0; r0 < H4; r0 += CF_ROWS) {
        __syncthreads();                                   // the previous chunk is consumed (first time: nothing)
        for (int r = wave; r < CF_ROWS; r += CF_THREADS / 64) {
            const int i = r0 + r;
            for (int j = lane; j < W4; j += 64) s_x[r * xs + j] = (i < H && j < W) ? xp[(size_t)i * W + j] : 0.f;
        }
        __syncthreads();
        const int i = r0 + rr;
        if (i < H4 && c0 + cq < W) {
            float o[4] = {0.f, 0.f, 0.f, 0.f};             // rows H .. H4-1 of s_t are the column pass's zero padding
            if (i < H) cf_dot<4>(s_x + rr * xs, W4, s_th, c0 + cq + W4, o);
#pragma unroll
            for (int k = 0; k < 4; ++k) s_t[(cq + k) * ts + i] = o[k];
        }
    }
    __syncthreads();

    // column pass: y[i][c0 + c] = sum_r cv[(i - r) mod H] * s_t[c][r]
    const int c = tid & 31;
    if (c0 + c < W) {
        float *yp = y + (size_t)plane * H * W + c0 + c;
        const int nib = (H + 7) >> 3;
        for (int ib = tid >> 5; ib < nib; ib += CF_THREADS / 32) {
            float o[8];
            cf_dot<8>(s_t + c * ts, H4, s_tv, 8 * ib + H4, o);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (8 * ib + k < H) yp[(size_t)(8 * ib + k) * W] = o[k];
        }
    }
}

// pick a tile so that tile + halo fits comfortably in LDS and small images are one tile
inline void blur_tiles(int H, int W, int kv, int kh, int &th, int &tw) {
    th = H < 64 ? H : 64;
    tw = W < 64 ? W : 64;
    (void)kv; (void)kh;
}

}  // namespace

// By HIP's contract a launch with more than 64 KiB of dynamic LDS needs the kernel's allowance raised first. (The ROCm 7
// runtime on an MI355X was seen to launch resample_sepband_kernel and blur_sep_circ_kernel at 66 to 153 KiB without it,
// with right results; the code keeps to the contract, not to that.) It is raised once per device (to the 160 KiB of a
// CU), on the first such call there -- an eager one, ahead of any capture of the same extent -- and remembered in one bit
// per (kernel, device): idempotent, so a race between two first calls only repeats it.
constexpr size_t LDS_DEFAULT = 64 * 1024, LDS_MAX = 160 * 1024;

struct BigLdsKernel {
    const void *kernel;
    std::atomic<unsigned long long> devices{0};
};
static BigLdsKernel big_lds_blur_sep{reinterpret_cast<const void *>(blur_sep_circ_kernel)};
static BigLdsKernel big_lds_resample{reinterpret_cast<const void *>(resample_sepband_kernel)};
static BigLdsKernel big_lds_circ_filter{reinterpret_cast<const void *>(circ_filter_sep_kernel)};

static int allow_big_lds(BigLdsKernel &k, size_t lds) {
    if (lds <= LDS_DEFAULT) return 0;
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return (int)e;
    const unsigned long long bit = 1ull << (device & 63);
    if (k.devices.load(std::memory_order_relaxed) & bit) return 0;
    e = hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX);
    if (e != hipSuccess) return (int)e;
    k.devices.fetch_or(bit, std::memory_order_relaxed);
    return 0;
}

// The launch sei_blur_sep_circ makes: tile and dynamic LDS bytes (0: refused).
struct BlurSepLaunch {
    int tile_h, tile_w;
    size_t lds;
};
static BlurSepLaunch blur_sep_launch(int kv, int kh, int H, int W) {
    BlurSepLaunch l{0, 0, 0};
    if (H <= 0 || W <= 0 || kv <= 0 || kh <= 0 || kv > MAX_TAPS || kh > MAX_TAPS) return l;
    blur_tiles(H, W, kv, kh, l.tile_h, l.tile_w);
    const int ih = l.tile_h + kv - 1, iw = l.tile_w + kh - 1;
    const size_t lds = sizeof(float) * (128 + ((ih * iw + 3) & ~3) + (size_t)ih * l.tile_w);
    if (lds <= LDS_MAX) l.lds = lds;
    return l;
}

extern "C" size_t sei_blur_sep_circ_lds(int kv, int kh, int H, int W) { return blur_sep_launch(kv, kh, H, W).lds; }

extern "C" int sei_blur_sep_circ(const float *x, float *y, const float *tv, const float *th, int kv,
                                 int kh, int planes, int H, int W, int transpose, void *stream) {
    SEI_REQUIRE(x && y && tv && th && x != y);
    SEI_REQUIRE(planes > 0 && H > 0 && W > 0 && kv > 0 && kh > 0);
    const BlurSepLaunch l = blur_sep_launch(kv, kh, H, W);
    if (l.lds == 0) return SEI_ERR_TOO_LARGE;
    const int tiles_y = (int)sei_ceil_div(H, l.tile_h), tiles_x = (int)sei_ceil_div(W, l.tile_w);
    // forward: shift kv/2, taps as given; adjoint: flipped taps, shift kv-1-kv/2
    const int sv = transpose ? kv - 1 - kv / 2 : kv / 2, sh = transpose ? kh - 1 - kh / 2 : kh / 2;
    const size_t grid = (size_t)planes * tiles_y * tiles_x;
    const int rc = allow_big_lds(big_lds_blur_sep, l.lds);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(blur_sep_circ_kernel, dim3((unsigned)grid), dim3(BLUR_THREADS), l.lds, (hipStream_t)stream,
                       x, y, tv, th, kv, kh, sv, sh, transpose ? 1 : 0, H, W, l.tile_h, l.tile_w, tiles_y, tiles_x);
    return sei_launch_status();
}

extern "C" int sei_blur_dense_circ(const float *x, float *y, const float *k, int kv, int kh, int planes,
                                   int H, int W, int transpose, void *stream) {
    SEI_REQUIRE(x && y && k && x != y);
    SEI_REQUIRE(planes > 0 && H > 0 && W > 0 && kv > 0 && kh > 0);
    if (kv > MAX_TAPS || kh > MAX_TAPS) return SEI_ERR_TOO_LARGE;
    int tile_h = H < 32 ? H : 32, tile_w = W < 64 ? W : 64;
    const int tiles_y = (int)sei_ceil_div(H, tile_h), tiles_x = (int)sei_ceil_div(W, tile_w);
    const int ih = tile_h + kv - 1, iw = tile_w + kh - 1;
    const size_t lds = sizeof(float) * (((kv * kh + 3) & ~3) + (size_t)ih * iw);
    if (lds > LDS_MAX) return SEI_ERR_TOO_LARGE;
    const int sv = transpose ? kv - 1 - kv / 2 : kv / 2, sh = transpose ? kh - 1 - kh / 2 : kh / 2;
    const size_t grid = (size_t)planes * tiles_y * tiles_x;
    hipLaunchKernelGGL(blur_dense_circ_kernel, dim3((unsigned)grid), dim3(BLUR_THREADS), lds, (hipStream_t)stream,
                       x, y, k, kv, kh, sv, sh, transpose ? 1 : 0, H, W, tile_h, tile_w, tiles_y, tiles_x);
    return sei_launch_status();
}

// The launches sei_blur_dense_pad makes. One axis of K taps reads s positions before its output and K-1-s after it, of
// an image padded by p: (K/2, K/2) for odd K >= 3, (K/2 - 1, K/2) for even K, (0, 1) for K = 1 (sei_hip.h).
struct BlurPadPlan {
    int Hi, Wi, Ho, Wo;      // extents the tiled kernel reads and writes (its output is Z when `fold`)
    int sv, sh, flip, stage; // shifts, tap order and staging map of the tiled kernel
    int pv, ph;
    bool fold;
    size_t work;             // floats of Z (0: the tiled kernel writes y)
};
static int blur_pad_plan(int planes, int H, int W, int kv, int kh, int mode, int transpose, BlurPadPlan &pl) {
    SEI_REQUIRE(planes > 0 && H > 0 && W > 0 && kv > 0 && kh > 0);
    SEI_REQUIRE(mode == PAD_REPLICATE || mode == PAD_REFLECT || mode == PAD_VALID);
    if (kv > MAX_TAPS || kh > MAX_TAPS || H > (1 << 30) || W > (1 << 30)) return SEI_ERR_TOO_LARGE;
    int sv, sh;
    blur_pad_axis(kv, sv, pl.pv);
    blur_pad_axis(kh, sh, pl.ph);
    if (mode == PAD_REFLECT) SEI_REQUIRE(pl.pv <= H - 1 && pl.ph <= W - 1);
    if (mode == PAD_VALID) SEI_REQUIRE(H > 2 * pl.pv && W > 2 * pl.ph);
    pl.Hi = pl.Ho = H, pl.Wi = pl.Wo = W;
    pl.fold = false, pl.work = 0;
    if (!transpose) {
        pl.flip = 0, pl.stage = mode;
        pl.sv = sv, pl.sh = sh;
        if (mode == PAD_VALID) pl.Ho = H - 2 * pl.pv, pl.Wo = W - 2 * pl.ph, pl.sv += pl.pv, pl.sh += pl.ph;
    } else {
        pl.flip = 1, pl.stage = PAD_ZERO;
        pl.sv = kv - 1 - pl.pv - sv, pl.sh = kh - 1 - pl.ph - sh;
        if (mode == PAD_VALID) {
            pl.Hi = H - 2 * pl.pv, pl.Wi = W - 2 * pl.ph;    // Z of the cropped image is the whole result
        } else {
            pl.Ho = H + 2 * pl.pv, pl.Wo = W + 2 * pl.ph;
            pl.fold = true;
            pl.work = (size_t)planes * pl.Ho * pl.Wo;
        }
    }
    const size_t tiles = sei_ceil_div(pl.Ho, 32) * sei_ceil_div(pl.Wo, 64);
    if ((size_t)planes * tiles >= ((size_t)1 << 31) || sei_ceil_div((size_t)planes * H * W, 256) >= ((size_t)1 << 31))
        return SEI_ERR_TOO_LARGE;
    return 0;
}

template <int MODE>
static void blur_dense_pad_launch(const float *x, float *y, const float *k, int kv, int kh, int planes,
                                  const BlurPadPlan &pl, hipStream_t stream) {
    const int tile_h = pl.Ho < 32 ? pl.Ho : 32, tile_w = pl.Wo < 64 ? pl.Wo : 64;
    const int tiles_y = (int)sei_ceil_div(pl.Ho, tile_h), tiles_x = (int)sei_ceil_div(pl.Wo, tile_w);
    const int ih = tile_h + kv - 1, iw = tile_w + kh - 1;
    const size_t lds = sizeof(float) * (((kv * kh + 3) & ~3) + (size_t)ih * iw);      // <= 63 KiB at 63 x 63 taps
    const size_t grid = (size_t)planes * tiles_y * tiles_x;
    hipLaunchKernelGGL(blur_dense_pad_kernel<MODE>, dim3((unsigned)grid), dim3(BLUR_THREADS), lds, stream, x, y, k, kv, kh,
                       pl.sv, pl.sh, pl.flip, pl.Hi, pl.Wi, pl.Ho, pl.Wo, tile_h, tile_w, tiles_y, tiles_x);
}

extern "C" size_t sei_blur_dense_pad_work_floats(int planes, int H, int W, int kv, int kh, int mode, int transpose) {
    BlurPadPlan pl;
    return blur_pad_plan(planes, H, W, kv, kh, mode, transpose, pl) == 0 ? pl.work : 0;
}

extern "C" int sei_blur_dense_pad(const float *x, float *y, const float *k, int kv, int kh, int planes, int H, int W,
                                  int mode, int transpose, float *work, void *stream) {
    SEI_REQUIRE(x && y && k);
    BlurPadPlan pl;
    const int rc = blur_pad_plan(planes, H, W, kv, kh, mode, transpose, pl);
    if (rc != 0) return rc;
    SEI_REQUIRE(pl.work == 0 || work);
    // x and y at the image's extent or, in `valid`, the cropped one on the side the direction puts it
    const size_t full = (size_t)planes * H * W, crop = (size_t)planes * (H - 2 * pl.pv) * (W - 2 * pl.ph);
    const size_t nx = mode == PAD_VALID && transpose ? crop : full, ny = mode == PAD_VALID && !transpose ? crop : full;
    const size_t nk = (size_t)kv * kh;
    SEI_REQUIRE(!floats_overlap(x, nx, y, ny) && !floats_overlap(k, nk, y, ny));
    if (pl.work) SEI_REQUIRE(!floats_overlap(x, nx, work, pl.work) && !floats_overlap(y, ny, work, pl.work) &&
                             !floats_overlap(k, nk, work, pl.work));
    hipStream_t s = (hipStream_t)stream;
    float *dst = pl.fold ? work : y;
    switch (pl.stage) {
    case PAD_REPLICATE: blur_dense_pad_launch<PAD_REPLICATE>(x, dst, k, kv, kh, planes, pl, s); break;
    case PAD_REFLECT: blur_dense_pad_launch<PAD_REFLECT>(x, dst, k, kv, kh, planes, pl, s); break;
    case PAD_VALID: blur_dense_pad_launch<PAD_VALID>(x, dst, k, kv, kh, planes, pl, s); break;
    default: blur_dense_pad_launch<PAD_ZERO>(x, dst, k, kv, kh, planes, pl, s); break;
    }
    if (pl.fold) {
        const int status = sei_launch_status();
        if (status != 0) return status;
        return sei_blur_pad_fold_launch(mode, work, y, planes, H, W, pl.pv, pl.ph, s);
    }
    return sei_launch_status();
}

int sei_blur_pad_fold_launch(int mode, const float *Z, float *out, int planes, int H, int W, int pv, int ph, hipStream_t s) {
    const size_t full = (size_t)planes * H * W;
    const unsigned grid = (unsigned)sei_ceil_div(full, 256);
    if (mode == PAD_REPLICATE)
        hipLaunchKernelGGL(blur_pad_fold_kernel<PAD_REPLICATE>, dim3(grid), dim3(256), 0, s, Z, out, H, W, pv, ph, full);
    else
        hipLaunchKernelGGL(blur_pad_fold_kernel<PAD_REFLECT>, dim3(grid), dim3(256), 0, s, Z, out, H, W, pv, ph, full);
    return sei_launch_status();
}

// LDS bytes of one circ_filter_sep_kernel workgroup (the layout in the kernel's comment)
static size_t circ_filter_lds(int H, int W) {
    const int H4 = (H + 3) & ~3, W4 = (W + 3) & ~3;
    const size_t len_h = (size_t)((W + CF_STRIP - 1) & ~(CF_STRIP - 1)) + W4, len_v = (size_t)((H + 7) & ~7) + H4;
    return sizeof(float) * (len_h + len_v + (size_t)CF_ROWS * cf_stride(W4) + (size_t)CF_STRIP * cf_stride(H4));
}

extern "C" int sei_circ_filter_sep(const float *x, float *y, const float *cv, const float *ch, int planes, int H,
                                   int W, void *stream) {
    SEI_REQUIRE(x && y && cv && ch && x != y);
    SEI_REQUIRE(planes > 0 && H > 0 && W > 0);
    if (H > (1 << 15) || W > (1 << 15)) return SEI_ERR_TOO_LARGE;
    const size_t lds = circ_filter_lds(H, W);
    if (lds > LDS_MAX) return SEI_ERR_TOO_LARGE;
    const int strips = (int)sei_ceil_div(W, CF_STRIP);
    const size_t grid = (size_t)planes * strips;
    if (grid >= ((size_t)1 << 31)) return SEI_ERR_TOO_LARGE;
    const int rc = allow_big_lds(big_lds_circ_filter, lds);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(circ_filter_sep_kernel, dim3((unsigned)grid), dim3(CF_THREADS), lds, (hipStream_t)stream, x, y,
                       cv, ch, H, W, strips);
    return sei_launch_status();
}

// The launch sei_resample_sepband makes: output tile, the LDS footprint bound of its input, dynamic LDS bytes (0: refused).
// Output tile 16 x 32; its input footprint is at most (tile-1)*step + band per axis. Where that asks for more LDS than a
// CU has (reductions by 8 and more), the tile is halved, the wider footprint first, until it fits.
struct ResampleLaunch {
    int tile_h, tile_w, fh_max, fw_max;
    size_t lds;
};
static ResampleLaunch resample_launch(int Hi, int Wi, int Ho, int Wo, int nbv, int stepv, int nbh, int steph) {
    ResampleLaunch l{0, 0, 0, 0, 0};
    if (Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0 || nbv <= 0 || nbh <= 0 || stepv < 0 || steph < 0) return l;
    l.tile_h = Ho < 16 ? Ho : 16;
    l.tile_w = Wo < 32 ? Wo : 32;
    for (;;) {
        // (64-bit: a step is below the input extent, so a footprint bound is below 32 extents)
        const long long fh = (long long)(l.tile_h - 1) * stepv + nbv, fw = (long long)(l.tile_w - 1) * steph + nbh;
        l.fh_max = (int)(fh < Hi ? fh : Hi);
        l.fw_max = (int)(fw < Wi ? fw : Wi);
        const size_t lds = sizeof(float) * ((((size_t)l.fh_max * l.fw_max + 3) & ~(size_t)3) + (size_t)l.fh_max * l.tile_w);
        if (lds <= LDS_MAX) {
            l.lds = lds;
            return l;
        }
        if (l.tile_w > 1 && (l.fw_max >= l.fh_max || l.tile_h == 1)) l.tile_w = (l.tile_w + 1) / 2;
        else if (l.tile_h > 1) l.tile_h = (l.tile_h + 1) / 2;
        else return l;                                  // one output pixel's own bands do not fit
    }
}

extern "C" size_t sei_resample_sepband_lds(int Hi, int Wi, int Ho, int Wo, int nbv, int stepv, int nbh, int steph) {
    return resample_launch(Hi, Wi, Ho, Wo, nbv, stepv, nbh, steph).lds;
}

extern "C" int sei_resample_sepband(const float *x, float *y, int planes, int Hi, int Wi, int Ho, int Wo,
                                    const float *wv, const int *lov, int nbv, int stepv,
                                    const float *wh, const int *loh, int nbh, int steph, void *stream) {
    SEI_REQUIRE(x && y && wv && lov && wh && loh && x != y);
    SEI_REQUIRE(planes > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && nbv > 0 && nbh > 0);
    SEI_REQUIRE(stepv >= 0 && steph >= 0);
    const ResampleLaunch l = resample_launch(Hi, Wi, Ho, Wo, nbv, stepv, nbh, steph);
    if (l.lds == 0) return SEI_ERR_TOO_LARGE;
    const int tiles_y = (int)sei_ceil_div(Ho, l.tile_h), tiles_x = (int)sei_ceil_div(Wo, l.tile_w);
    const size_t grid = (size_t)planes * tiles_y * tiles_x;
    if (grid >= ((size_t)1 << 31)) return SEI_ERR_TOO_LARGE;
    const int rc = allow_big_lds(big_lds_resample, l.lds);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(resample_sepband_kernel, dim3((unsigned)grid), dim3(RS_THREADS), l.lds, (hipStream_t)stream,
                       x, y, Hi, Wi, Ho, Wo, wv, lov, nbv, wh, loh, nbh, l.tile_h, l.tile_w, tiles_y, tiles_x,
                       l.fh_max, l.fw_max);
    return sei_launch_status();
}

extern "C" int sei_scale_resample_fwd(const float *x, float *y, const float *rate, const float *center,
                                      int B, int C, int Hi, int Wi, int H, int W, void *stream) {
    SEI_REQUIRE(x && y && rate && center && x != y);
    SEI_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && Hi > 0 && Wi > 0);
    const size_t total = (size_t)B * H * W;
    // python: 2 / w evaluated in double, then rounded to float32 when it multiplies a float tensor
    const float two_over_h = (float)(2.0 / (double)H), two_over_w = (float)(2.0 / (double)W);
    hipLaunchKernelGGL(scale_resample_fwd_kernel, dim3((unsigned)sei_ceil_div(total, 256)), dim3(256), 0,
                       (hipStream_t)stream, x, y, rate, center, B, C, Hi, Wi, H, W, two_over_h, two_over_w);
    return sei_launch_status();
}

extern "C" int sei_scale_resample_bwd(const float *gy, float *gx, const float *rate, const float *center,
                                      int B, int C, int Hi, int Wi, int H, int W, void *stream) {
    SEI_REQUIRE(gy && gx && rate && center && gx != gy);
    SEI_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && Hi > 0 && Wi > 0);
    const size_t total = (size_t)B * H * W;
    const float two_over_h = (float)(2.0 / (double)H), two_over_w = (float)(2.0 / (double)W);
    hipLaunchKernelGGL(scale_resample_bwd_kernel, dim3((unsigned)sei_ceil_div(total, 256)), dim3(256), 0,
                       (hipStream_t)stream, gy, gx, rate, center, B, C, Hi, Wi, H, W, two_over_h, two_over_w);
    return sei_launch_status();
}

static RotateMap rotate_map(const float theta[4], int H, int W) {
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    return RotateMap{theta[0] / hw, theta[1] / hw, theta[2] / hh, theta[3] / hh};
}

extern "C" int sei_rotate_nearest_fwd(const float *x, float *y, int planes, int H, int W, float t00, float t01,
                                      float t10, float t11, void *stream) {
    SEI_REQUIRE(x && y && x != y && planes > 0 && H > 0 && W > 0 && (size_t)H * W < (1u << 30));
    const float theta[4] = {t00, t01, t10, t11};
    const dim3 grid((unsigned)sei_ceil_div((size_t)H * W, 256), (unsigned)(planes < 1024 ? planes : 1024));
    hipLaunchKernelGGL(rotate_nearest_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, y, planes, H, W,
                       rotate_map(theta, H, W));
    return sei_launch_status();
}

extern "C" int sei_rotate_nearest_bwd(const float *gy, float *gx, int planes, int H, int W, float t00, float t01,
                                      float t10, float t11, void *stream) {
    SEI_REQUIRE(gy && gx && gx != gy && planes > 0 && H > 0 && W > 0 && (size_t)H * W < (1u << 30));
    const float theta[4] = {t00, t01, t10, t11};
    const dim3 grid((unsigned)sei_ceil_div((size_t)H * W, 256), (unsigned)(planes < 1024 ? planes : 1024));
    hipLaunchKernelGGL(rotate_nearest_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, gy, gx, planes, H, W,
                       rotate_map(theta, H, W));
    return sei_launch_status();
}
