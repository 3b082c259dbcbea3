// Evaluation metrics for gfx950: the luma SSIM of a batch of image pairs (reference src/metrics.py:15-18: kornia
// rgb_to_ycbcr's Y, then torchmetrics structural_similarity_index_measure with its defaults and data_range 1).
//
//   ssim_tile_kernel : one workgroup per (64 x 32 tile of the SSIM map, image). The tile's luma plus its 10-pixel halo,
//                      for both images, goes to LDS; an 11-tap horizontal pass forms the five weighted moments of every
//                      halo row, the vertical pass the moments of every window, then the SSIM formula, and the tile's
//                      sum of the map goes to work[image][tile] with a plain store.
//   ssim_mean_kernel : one workgroup per image sums that image's tile sums in a fixed order, in double, and stores
//                      the mean of the map.
// No atomics: the result is bitwise reproducible and does not depend on the batch an image is evaluated in.
//
// Cancellation: sigma^2 = E[x^2] - mu^2 loses the digits that x's level and its local variation share. The luma of
// each tile is stored relative to the luma of one pixel of the tile (a per-tile shift c; variances and the covariance
// do not change under a shift, and mu = mu' + c restores the means), so a smooth region costs no more than a busy one.
#include "sei_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int TW = 64, TH = 32;                  // SSIM-map tile: one map column per lane, TH / 4 map rows per wave
constexpr int TAPS = 11, HALO = TAPS - 1;
constexpr int RW = TW + HALO, RH = TH + HALO;    // the 74 x 42 luma region a tile reads
constexpr int LP = RW + 1;                       // luma row pitch in LDS
constexpr int ROWS = TH / (THREADS / 64);        // map rows per wave (8)
constexpr int LOAD_ITERS = (RH * RW + THREADS - 1) / THREADS;
constexpr int LDS_FLOATS = 2 * RH * LP + 5 * RH * TW;   // 78,960 bytes: two workgroups per CU

struct Taps {
    float g[TAPS];
};

__device__ __forceinline__ float luma_at(const float *__restrict__ p, size_t i, size_t plane) {
    return 0.299f * p[i] + 0.587f * p[plane + i] + 0.114f * p[2 * plane + i];      // luma_sqerr_kernel's constants
}

// moments m = (mu_a, mu_b, E[a^2], E[b^2], E[ab]) of the shifted values a - ca, b - cb
__device__ __forceinline__ float ssim_value(const float (&m)[5], float ca, float cb) {
    const float C1 = 0.0001f, C2 = 0.0009f;                                    // (0.01 * 1)^2, (0.03 * 1)^2
    const float va = fmaxf(m[2] - m[0] * m[0], 0.f);
    const float vb = fmaxf(m[3] - m[1] * m[1], 0.f);
    const float cov = m[4] - m[0] * m[1];
    const float mua = m[0] + ca, mub = m[1] + cb;
    const float num = (2.f * mua * mub + C1) * (2.f * cov + C2);
    const float den = (mua * mua + mub * mub + C1) * (va + vb + C2);
    return num / den;
}

__global__ __launch_bounds__(THREADS) void ssim_tile_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                            int H, int W, int tiles_x, int tiles, Taps taps,
                                                            float *__restrict__ work) {
    __shared__ float lds[LDS_FLOATS];
    __shared__ float scratch[THREADS / 64];
    float *la = lds, *lb = lds + RH * LP;        // shifted luma, [RH][LP]
    float *mom = lds + 2 * RH * LP;              // horizontal moments, [5][RH][TW]
    const int tile = blockIdx.x, img = blockIdx.y;
    const int ty0 = (tile / tiles_x) * TH, tx0 = (tile % tiles_x) * TW;
    const size_t plane = (size_t)H * W;
    const float *pa = a + (size_t)img * 3 * plane, *pb = b + (size_t)img * 3 * plane;

    // the tile's shift: the luma at the centre of its region, clamped into the image (every thread reads it)
    const size_t ci = (size_t)min(ty0 + RH / 2, H - 1) * W + min(tx0 + RW / 2, W - 1);
    const float ca = luma_at(pa, ci, plane), cb = luma_at(pb, ci, plane);

    // A fixed trip count, unrolled, and no load under a condition: every load of the region is issued before the first
    // LDS store waits for one. Positions beyond the image read the nearest image pixel (in bounds); they feed only map
    // entries that are not summed.
#pragma unroll
    for (int it = 0; it < LOAD_ITERS; ++it) {
        const int i = min(it * THREADS + (int)threadIdx.x, RH * RW - 1);
        const int r = i / RW, c = i - r * RW;
        const size_t p = (size_t)min(ty0 + r, H - 1) * W + min(tx0 + c, W - 1);
        const float va = luma_at(pa, p, plane) - ca, vb = luma_at(pb, p, plane) - cb;
        if (it * THREADS + (int)threadIdx.x < RH * RW) {
            la[r * LP + c] = va;
            lb[r * LP + c] = vb;
        }
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < RH; r += THREADS / 64) {
        float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
            const float x = la[r * LP + lane + k], y = lb[r * LP + lane + k], g = taps.g[k];
            m0 = fmaf(g, x, m0);
            m1 = fmaf(g, y, m1);
            m2 = fmaf(g, x * x, m2);
            m3 = fmaf(g, y * y, m3);
            m4 = fmaf(g, x * y, m4);
        }
        mom[(0 * RH + r) * TW + lane] = m0;
        mom[(1 * RH + r) * TW + lane] = m1;
        mom[(2 * RH + r) * TW + lane] = m2;
        mom[(3 * RH + r) * TW + lane] = m3;
        mom[(4 * RH + r) * TW + lane] = m4;
    }
    __syncthreads();

    // vertical pass: map rows r0 .. r0 + ROWS - 1 of column `lane` read halo rows r0 .. r0 + ROWS + HALO - 1 once each
    const int r0 = wave * ROWS;
    float acc[ROWS][5];
#pragma unroll
    for (int o = 0; o < ROWS; ++o)
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[o][q] = 0.f;
#pragma unroll
    for (int j = 0; j < ROWS + HALO; ++j) {
        float v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = mom[(q * RH + r0 + j) * TW + lane];
#pragma unroll
        for (int o = 0; o < ROWS; ++o) {
            const int k = j - o;                 // tap k of map row r0 + o (taps in increasing order, as horizontally)
            if (k >= 0 && k < TAPS) {
#pragma unroll
                for (int q = 0; q < 5; ++q) acc[o][q] = fmaf(taps.g[k], v[q], acc[o][q]);
            }
        }
    }
    float s = 0.f;
    const bool col_in = tx0 + lane < W - HALO;
#pragma unroll
    for (int o = 0; o < ROWS; ++o)
        if (col_in && ty0 + r0 + o < H - HALO) s += ssim_value(acc[o], ca, cb);
    const float t = sei_block_sum<THREADS>(s, scratch);
    if (threadIdx.x == 0) work[(size_t)img * tiles + tile] = t;
}

__global__ __launch_bounds__(THREADS) void ssim_mean_kernel(const float *__restrict__ work, int tiles, double count,
                                                            float *__restrict__ out) {
    __shared__ double scratch[THREADS / 64];
    const float *w = work + (size_t)blockIdx.x * tiles;
    double s = 0.0;
    for (int i = threadIdx.x; i < tiles; i += THREADS) s += (double)w[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int i = 0; i < THREADS / 64; ++i) total += scratch[i];
        out[blockIdx.x] = (float)(total / count);
    }
}

bool ssim_geometry(int batch, int H, int W, int &tiles_x, int &tiles) {
    if (batch < 1 || batch > 65535 || H < TAPS || W < TAPS || (size_t)H * W >= ((size_t)1 << 30)) return false;
    tiles_x = (int)sei_ceil_div(W - HALO, TW);
    tiles = tiles_x * (int)sei_ceil_div(H - HALO, TH);
    return true;
}

}  // namespace

extern "C" size_t sei_ssim_luma_work_floats(int batch, int H, int W) {
    int tiles_x, tiles;
    if (!ssim_geometry(batch, H, W, tiles_x, tiles)) return 0;
    return (size_t)batch * tiles;
}

extern "C" int sei_ssim_luma(const float *a, const float *b, int batch, int H, int W, float *out, float *work,
                             void *stream) {
    SEI_REQUIRE(a && b && out && work);
    int tiles_x, tiles;
    SEI_REQUIRE(ssim_geometry(batch, H, W, tiles_x, tiles));
    // torchmetrics' _gaussian(11, 1.5): exp(-(i / 1.5)^2 / 2), i = -5 .. 5, normalised to sum 1
    Taps taps;
    double g[TAPS], sum = 0.0;
    for (int k = 0; k < TAPS; ++k) {
        const double d = (k - TAPS / 2) / 1.5;
        g[k] = exp(-0.5 * d * d);
        sum += g[k];
    }
    for (int k = 0; k < TAPS; ++k) taps.g[k] = (float)(g[k] / sum);
    hipLaunchKernelGGL(ssim_tile_kernel, dim3(tiles, batch), dim3(THREADS), 0, (hipStream_t)stream, a, b, H, W, tiles_x,
                       tiles, taps, work);
    const double count = (double)(H - HALO) * (double)(W - HALO);
    hipLaunchKernelGGL(ssim_mean_kernel, dim3(batch), dim3(THREADS), 0, (hipStream_t)stream, (const float *)work, tiles,
                       count, out);
    return sei_launch_status();
}
