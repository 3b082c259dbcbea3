// LPIPS v0.1 on AlexNet features for gfx950, float32 throughout (reference src/metrics.py: pyiqa.create_metric("lpips");
// the arithmetic is restated in metrics.py's host path and in include/sei_hip.h).
//
//   lpips_conv_relu_kernel : convolution + bias + ReLU as an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact float32, as
//                            gemm_f32.hip): M = output pixels of one image, N = Cout, K = k * k * Cin. One workgroup = 4
//                            waves = a 128 x 64 output tile (each wave 64 x 32: two 32 x 32 accumulators), K walked in
//                            tiles of 32 that are prefetched into registers under the MFMAs of the tile before. Both
//                            operands are K-contiguous in LDS (row stride 36 floats, ds_read_b128): activations are
//                            channels-last, so the 32 k of a tile are 32 consecutive channels of ONE tap, and the
//                            weights come repacked as [Cout][K]. Runtime kernel size / stride / padding: the same
//                            kernel serves 11 / 4, 5 / 1 and 3 / 1. FIRST = true swaps the A loader only: planar RGB
//                            input, K = (ci, ky, kx), LPIPS' input scaling applied to every in-image tap on load and
//                            0 (not scaled(0)) for the taps in the zero padding.
//                            Summation: the MFMA is a k-ordered fmaf chain, so a plain accumulator is a chain of up to
//                            3456 roundings; every 8 k-tiles (256 k) the chain is closed into a second accumulator, which
//                            keeps the error near that of blocked host sums.
//   lpips_maxpool_kernel   : 3 x 3 stride-2 max-pool, floor mode, channels-last, a float4 of channels per thread.
//   lpips_dist_kernel      : one wave per pixel, channels on the lanes: the two channel norms by a butterfly, then
//                            sum_c w[c] (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2, summed per lane over the wave's
//                            pixels, per workgroup in a fixed tree, stored to partials[image][workgroup].
//   lpips_dist_finish_kernel: one workgroup per image adds that image's partials in index order in double and stores
//                            (or adds to the running sum over the layers) the pixel mean.
// No atomics; the grids depend on the extents only, never on the batch: an image's value is the same bits in any batch.
#include "sei_common.h"

namespace {

constexpr int LP_BM = 128, LP_BN = 64, LP_BK = 32, LP_LD = LP_BK + 4, LP_THREADS = 256;
constexpr int LP_CHUNK = 8;                        // k-tiles per closed summation chain
constexpr int LP_DIST_THREADS = 256, LP_DIST_MAXJ = 6, LP_DIST_MAX_WG = 1024;

// ---- geometry of the five tapped layers for an H x W image ------------------------------------------------------
struct LayerGeom {
    int Hin, Win, Cin, Hout, Wout, Cout, ks, stride, pad;
};
struct Geom {
    LayerGeom conv[5];
    int pool_h[2], pool_w[2];                      // extents after the pool that follows conv1 / conv2
};

bool lpips_geometry(int n, int H, int W, Geom &g) {
    if (n < 1 || n > 32767 || H < 31 || W < 31 || H > 32768 || W > 32768 || (size_t)H * W > ((size_t)1 << 28)) return false;
    static const int cin[5] = {3, 64, 192, 384, 256}, cout[5] = {64, 192, 384, 256, 256};
    static const int ks[5] = {11, 5, 3, 3, 3}, stride[5] = {4, 1, 1, 1, 1}, pad[5] = {2, 2, 1, 1, 1};
    int h = H, w = W;
    for (int l = 0; l < 5; ++l) {
        LayerGeom &c = g.conv[l];
        c.Hin = h, c.Win = w, c.Cin = cin[l], c.Cout = cout[l], c.ks = ks[l], c.stride = stride[l], c.pad = pad[l];
        c.Hout = (h + 2 * pad[l] - ks[l]) / stride[l] + 1;
        c.Wout = (w + 2 * pad[l] - ks[l]) / stride[l] + 1;
        h = c.Hout, w = c.Wout;
        if (l < 2) {                               // maxpool(3, stride 2), floor mode, no padding
            h = (h - 3) / 2 + 1, w = (w - 3) / 2 + 1;
            g.pool_h[l] = h, g.pool_w[l] = w;
        }
    }
    return true;
}

inline int dist_workgroups(size_t P, int &pix_per_wg) {
    size_t nwg = sei_ceil_div(P, 16);
    if (nwg > LP_DIST_MAX_WG) nwg = LP_DIST_MAX_WG;
    pix_per_wg = (int)sei_ceil_div(P, nwg);
    return (int)sei_ceil_div(P, (size_t)pix_per_wg);
}

// ---- convolution + bias + ReLU ---------------------------------------------------------------------------------
struct ConvArgs {
    const float *x, *x2;                           // FIRST: images [0, split) from x, [split, n) from x2
    const float *w, *bias;                         // w: [Cout][Kpad]
    float *y;                                      // [image][Hout * Wout][Cout]
    int split, Kpad;
    LayerGeom g;
};

__device__ __forceinline__ float lpips_scaled(float raw, int ci) {
    // lpips' normalize=True (2 x - 1), then its ScalingLayer
    const float shift = ci == 0 ? -0.030f : (ci == 1 ? -0.088f : -0.188f);
    const float scale = ci == 0 ? 0.458f : (ci == 1 ? 0.448f : 0.450f);
    return ((2.f * raw - 1.f) - shift) / scale;
}

template <bool FIRST>
__global__ __launch_bounds__(LP_THREADS) void lpips_conv_relu_kernel(ConvArgs a) {
    __shared__ __attribute__((aligned(16))) float As[LP_BM * LP_LD];
    __shared__ __attribute__((aligned(16))) float Bs[LP_BN * LP_LD];
    const LayerGeom g = a.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
    // column tiles vary fastest: the workgroups that share an A tile are neighbours in dispatch order
    const int ntn = g.Cout / LP_BN;
    const int n0 = (blockIdx.x % ntn) * LP_BN, m0 = (blockIdx.x / ntn) * LP_BM, img = blockIdx.y;
    const int P = g.Hout * g.Wout;
    const int Hin = g.Hin, Win = g.Win, Cin = g.Cin, ks = g.ks, Kpad = a.Kpad;
    const float *__restrict__ wgt = a.w;
    const float *__restrict__ xin;
    if (FIRST)
        xin = img < a.split ? a.x + (size_t)img * 3 * Hin * Win : a.x2 + (size_t)(img - a.split) * 3 * Hin * Win;
    else
        xin = a.x + (size_t)img * Hin * Win * Cin;

    // The output pixels this thread stages: FIRST -- one pixel (tid % 128) and 16 consecutive k (half tid / 128) of every
    // tile; otherwise four pixels (tid / 8 + 32 it) and one float4 of channels ((tid % 8) * 4). A pixel beyond the image's
    // last one gets a row far outside, so that its taps fail the bounds test and stage zeros.
    constexpr int NPIX = FIRST ? 1 : 4;
    int iy0[NPIX], ix0[NPIX];
#pragma unroll
    for (int it = 0; it < NPIX; ++it) {
        const int m = m0 + (FIRST ? (tid & 127) : (tid >> 3) + 32 * it);
        const int oy = m / g.Wout, ox = m - oy * g.Wout;
        iy0[it] = m < P ? oy * g.stride - g.pad : -(1 << 24);
        ix0[it] = ox * g.stride - g.pad;
    }
    const int k4 = (tid & 7) << 2;
    int ky = 0, kx = 0, c0 = 0;                    // tap and first channel of the NEXT tile to load (not FIRST)

    float4 ra[4], rb0, rb1;
    auto load_tile = [&](int k0) {
        if (FIRST) {
            int k = k0 + ((tid >> 7) << 4);
            int ci = k / (ks * ks);
            int r = k - ci * ks * ks;
            int fy = r / ks, fx = r - fy * ks;
            float v[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int iy = iy0[0] + fy, ix = ix0[0] + fx;
                float t = 0.f;                     // zero padding of the SCALED image, and the k beyond 3 * ks * ks
                if (ci < 3 && (unsigned)iy < (unsigned)Hin && (unsigned)ix < (unsigned)Win)
                    t = lpips_scaled(xin[((size_t)ci * Hin + iy) * Win + ix], ci);
                v[e] = t;
                if (++fx == ks) {
                    fx = 0;
                    if (++fy == ks) fy = 0, ++ci;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) ra[j] = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
        } else {
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int iy = iy0[it] + ky, ix = ix0[it] + kx;
                float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
                if ((unsigned)iy < (unsigned)Hin && (unsigned)ix < (unsigned)Win)
                    t = *reinterpret_cast<const float4 *>(xin + ((size_t)iy * Win + ix) * Cin + c0 + k4);
                ra[it] = t;
            }
            c0 += LP_BK;
            if (c0 == Cin) {
                c0 = 0;
                if (++kx == ks) kx = 0, ++ky;
            }
        }
        rb0 = *reinterpret_cast<const float4 *>(wgt + (size_t)(n0 + (tid >> 3)) * Kpad + k0 + k4);
        rb1 = *reinterpret_cast<const float4 *>(wgt + (size_t)(n0 + (tid >> 3) + 32) * Kpad + k0 + k4);
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            if (FIRST)
                *reinterpret_cast<float4 *>(As + (tid & 127) * LP_LD + ((tid >> 7) << 4) + 4 * it) = ra[it];
            else
                *reinterpret_cast<float4 *>(As + ((tid >> 3) + 32 * it) * LP_LD + k4) = ra[it];
        }
        *reinterpret_cast<float4 *>(Bs + (tid >> 3) * LP_LD + k4) = rb0;
        *reinterpret_cast<float4 *>(Bs + ((tid >> 3) + 32) * LP_LD + k4) = rb1;
    };

    f32x16 total[2], chain[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) total[i][r] = 0.f, chain[i][r] = 0.f;

    const int ntiles = Kpad / LP_BK;
    load_tile(0);
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();                           // the tile before is consumed
        store_tile();
        __syncthreads();
        if (t + 1 < ntiles) load_tile((t + 1) * LP_BK);   // in flight under this tile's MFMAs
        // step e of quarter q takes k = 4 q + e from lanes 0-31 and k = 16 + 4 q + e from lanes 32-63 (gemm_f32.hip)
#pragma unroll
        for (int q = 0; q < LP_BK / 8; ++q) {
            const float4 b4 = *reinterpret_cast<const float4 *>(Bs + (wn * 32 + li) * LP_LD + lh * (LP_BK / 2) + 4 * q);
            const float4 a0 = *reinterpret_cast<const float4 *>(As + (wm * 64 + li) * LP_LD + lh * (LP_BK / 2) + 4 * q);
            const float4 a1 = *reinterpret_cast<const float4 *>(As + (wm * 64 + 32 + li) * LP_LD + lh * (LP_BK / 2) + 4 * q);
#define SEI_LP_STEP(E)                                                                      \
            chain[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.E, b4.E, chain[0], 0, 0, 0); \
            chain[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.E, b4.E, chain[1], 0, 0, 0);
            SEI_LP_STEP(x) SEI_LP_STEP(y) SEI_LP_STEP(z) SEI_LP_STEP(w)
#undef SEI_LP_STEP
        }
        if ((t % LP_CHUNK) == LP_CHUNK - 1 || t + 1 == ntiles) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) total[i][r] += chain[i][r], chain[i][r] = 0.f;
        }
    }

    // C/D map: column = lane & 31 (Cout), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (pixel)
    const int col = n0 + wn * 32 + li;
    const float bias = a.bias[col];
    float *__restrict__ yimg = a.y + (size_t)img * P * g.Cout;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = m0 + wm * 64 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (row < P) yimg[(size_t)row * g.Cout + col] = fmaxf(total[i][r] + bias, 0.f);
        }
}

// ---- 3 x 3 stride-2 max-pool, channels-last ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void lpips_maxpool_kernel(const float *__restrict__ x, float *__restrict__ y, int Hin,
                                                            int Win, int Ho, int Wo, int C, size_t total4) {
    const int C4 = C >> 2;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total4; idx += (size_t)gridDim.x * 256) {
        const int c4 = (int)(idx % C4);
        const size_t p = idx / C4;
        const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
        const size_t n = p / ((size_t)Wo * Ho);
        // (2 oy + 2 <= Hin - 1 and 2 ox + 2 <= Win - 1 by the floor-mode extents: every tap is inside)
        const float *base = x + (((size_t)n * Hin + 2 * oy) * Win + 2 * ox) * C + 4 * c4;
        float4 m = *reinterpret_cast<const float4 *>(base);
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const float4 v = *reinterpret_cast<const float4 *>(base + ((size_t)dy * Win + dx) * C);
                m.x = fmaxf(m.x, v.x), m.y = fmaxf(m.y, v.y), m.z = fmaxf(m.z, v.z), m.w = fmaxf(m.w, v.w);
            }
        *reinterpret_cast<float4 *>(y + idx * 4) = m;
    }
}

// ---- per-layer distance -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LP_DIST_THREADS) void lpips_dist_kernel(const float *__restrict__ fa,
                                                                     const float *__restrict__ fb,
                                                                     const float *__restrict__ lin, int P, int C,
                                                                     int pix_per_wg, float *__restrict__ partials) {
    __shared__ float scratch[LP_DIST_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int img = blockIdx.y, nj = C >> 6;
    const float *pa = fa + (size_t)img * P * C + lane, *pb = fb + (size_t)img * P * C + lane;
    float wl[LP_DIST_MAXJ];
#pragma unroll
    for (int j = 0; j < LP_DIST_MAXJ; ++j) wl[j] = j < nj ? lin[lane + 64 * j] : 0.f;
    const int p_begin = blockIdx.x * pix_per_wg, p_end = min(P, p_begin + pix_per_wg);
    float acc = 0.f;
    for (int p = p_begin + wave; p < p_end; p += LP_DIST_THREADS / 64) {
        float va[LP_DIST_MAXJ], vb[LP_DIST_MAXJ], sa = 0.f, sb = 0.f;
#pragma unroll
        for (int j = 0; j < LP_DIST_MAXJ; ++j) {
            va[j] = j < nj ? pa[(size_t)p * C + 64 * j] : 0.f;
            vb[j] = j < nj ? pb[(size_t)p * C + 64 * j] : 0.f;
            sa += va[j] * va[j];
            sb += vb[j] * vb[j];
        }
        sa = sei_group_sum<64>(sa);                // every lane holds the same bits
        sb = sei_group_sum<64>(sb);
        const float da = sqrtf(sa) + 1e-10f, db = sqrtf(sb) + 1e-10f;
#pragma unroll
        for (int j = 0; j < LP_DIST_MAXJ; ++j) {
            const float d = va[j] / da - vb[j] / db;
            acc += wl[j] * (d * d);
        }
    }
    const float t = sei_block_sum<LP_DIST_THREADS>(acc, scratch);
    if (threadIdx.x == 0) partials[(size_t)img * gridDim.x + blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void lpips_dist_finish_kernel(const float *__restrict__ partials, int count,
                                                                double inv_pixels, float *__restrict__ out,
                                                                int accumulate) {
    __shared__ double scratch[256 / 64];
    const float *w = partials + (size_t)blockIdx.x * count;
    double s = 0.0;
    for (int i = threadIdx.x; i < count; i += 256) s += (double)w[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int i = 0; i < 256 / 64; ++i) total += scratch[i];
        const float d = (float)(total * inv_pixels);
        out[blockIdx.x] = accumulate ? out[blockIdx.x] + d : d;
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" size_t sei_lpips_work_floats(int batch, int H, int W) {
    Geom g;
    if (batch < 1 || batch > 16383 || !lpips_geometry(2 * batch, H, W, g)) return 0;
    size_t per_image = 0;
    for (int l = 0; l < 5; ++l) per_image += (size_t)g.conv[l].Hout * g.conv[l].Wout * g.conv[l].Cout;
    for (int l = 0; l < 2; ++l) per_image += (size_t)g.pool_h[l] * g.pool_w[l] * g.conv[l].Cout;
    return 2 * (size_t)batch * per_image + (size_t)batch * LP_DIST_MAX_WG;
}

extern "C" int sei_lpips_conv_relu(const float *x, const float *x2, int split, const float *w, const float *bias, float *y,
                                   int layer, int n, int H, int W, void *stream) {
    SEI_REQUIRE(x && w && bias && y && layer >= 0 && layer < 5);
    Geom geom;
    SEI_REQUIRE(lpips_geometry(n, H, W, geom));
    ConvArgs a;
    a.g = geom.conv[layer];
    a.x = x, a.x2 = x2, a.w = w, a.bias = bias, a.y = y, a.split = split;
    const int K = a.g.ks * a.g.ks * a.g.Cin;
    a.Kpad = (int)(sei_ceil_div(K, LP_BK) * LP_BK);
    SEI_REQUIRE(aligned16(w) && ((uintptr_t)bias & 3) == 0 && ((uintptr_t)y & 3) == 0);
    if (layer == 0) {
        SEI_REQUIRE(split >= 1 && split <= n && (split == n || x2) && ((uintptr_t)x & 3) == 0 && ((uintptr_t)x2 & 3) == 0);
    } else {
        SEI_REQUIRE(aligned16(x) && (const float *)y != x);
    }
    const size_t P = (size_t)a.g.Hout * a.g.Wout;
    const dim3 grid((unsigned)((a.g.Cout / LP_BN) * sei_ceil_div(P, LP_BM)), (unsigned)n);
    if (layer == 0)
        hipLaunchKernelGGL(lpips_conv_relu_kernel<true>, grid, dim3(LP_THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(lpips_conv_relu_kernel<false>, grid, dim3(LP_THREADS), 0, (hipStream_t)stream, a);
    return sei_launch_status();
}

extern "C" int sei_lpips_maxpool(const float *x, float *y, int layer, int n, int H, int W, void *stream) {
    SEI_REQUIRE(x && y && x != y && (layer == 0 || layer == 1) && aligned16(x) && aligned16(y));
    Geom geom;
    SEI_REQUIRE(lpips_geometry(n, H, W, geom));
    const LayerGeom &c = geom.conv[layer];
    const size_t total4 = (size_t)n * geom.pool_h[layer] * geom.pool_w[layer] * (c.Cout / 4);
    hipLaunchKernelGGL(lpips_maxpool_kernel, dim3(sei_capped_grid(total4, 256, 65535)), dim3(256), 0, (hipStream_t)stream, x, y,
                       c.Hout, c.Wout, geom.pool_h[layer], geom.pool_w[layer], c.Cout, total4);
    return sei_launch_status();
}

extern "C" int sei_lpips_layer_dist(const float *fa, const float *fb, const float *lin, int layer, int batch, int H, int W,
                                    float *out, int accumulate, float *work, void *stream) {
    SEI_REQUIRE(fa && fb && lin && out && work && layer >= 0 && layer < 5 && out != work);
    Geom geom;
    SEI_REQUIRE(lpips_geometry(batch, H, W, geom));
    const LayerGeom &c = geom.conv[layer];
    const size_t P = (size_t)c.Hout * c.Wout;
    int pix_per_wg;
    const int nwg = dist_workgroups(P, pix_per_wg);
    hipLaunchKernelGGL(lpips_dist_kernel, dim3(nwg, batch), dim3(LP_DIST_THREADS), 0, (hipStream_t)stream, fa, fb, lin, (int)P,
                       c.Cout, pix_per_wg, work);
    hipLaunchKernelGGL(lpips_dist_finish_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, (const float *)work, nwg,
                       1.0 / (double)P, out, accumulate ? 1 : 0);
    return sei_launch_status();
}
