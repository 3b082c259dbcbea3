// The classical super-resolution degradation for gfx950 (MI355X): blur, then keep every rate-th pixel, as one operator.
//
//   sei_blur_decimate : BlurDownsampling.A and its exact transpose (physics/blur_downsampling.py)
//
// Per axis of image length n, K taps c, rate s, phase o in [0, s), with the blur's own (map, S) (sei_hip.h):
//   forward    y[i'] = sum_a c[a] x[map(s i' + o - a + S)],                      i' in [0, n_out), n_out = ceil((n - o) / s)
//   transpose  out[u] = sum over (i', a) with map(s i' + o - a + S) == u of c[a] g[i']
// in two dimensions the tensor product over k[a,b]. Blurring at full resolution and slicing [o::s] computes s^2 times the
// taps that are kept and writes and re-reads a full-resolution intermediate; these kernels evaluate the kept samples only,
// and their transpose visits, per image pixel, only the taps whose residue mod s can reach it.
//
// Forward: the tiling of blur_dense_pad_kernel over MEASUREMENT pixels. The footprint of a tile, (tile - 1) s + K per
// axis, is staged through the boundary map (pad_fetch, blur_pad.h) DE-INTERLEAVED BY COLUMN PHASE: footprint column l
// lives at [l % s][l / s] of its row. Output column c reads, for tap b, footprint column s c + (kh-1-b): phase
// (kh-1-b) % s, index c + (kh-1-b) / s -- so for a given tap the lanes of a wave, which run along c, read consecutive
// dwords (a plain row-major footprint would be read s dwords apart: 2-way bank conflicts at s = 2, 4-way at s = 4).
// Transpose: a gather (no float atomics: the same bits on every run) of the zero-boundary correlation
//   Z[e,f] = sum_{a,b} k[a,b] g[(e + a - ov - Sv) / s, (f + b - oh - Sh) / s]     over the (a,b) that divide exactly,
// e, f canvas coordinates (the image extended by the halo), g zero outside the measurement. Consecutive lanes f share their
// g column in groups of s (a broadcast) and read s different taps. Replicate / reflect: Z on the canvas extended by p goes
// to `work`, then the family's blur_pad_fold_kernel. Circular: the fold is done in the kernel, out[u,v] = sum over wraps
// (mv, mh) of Z[u + mv H, v + mh W], one staging pass per wrap that the tile's taps reach (one for an interior tile; any
// number when the kernel is larger than the image), added in a fixed order.
// Both directions keep the family's accumulation order: each tap row summed on its own, the rows added in order.
#include "sei_common.h"
#include "blur_pad.h"

namespace {

constexpr int BD_THREADS = 256;
constexpr int BD_MAX_TAPS = 63, BD_MAX_RATE = 8;
constexpr size_t BD_LDS = 64 * 1024;           // the default dynamic-LDS allowance: no launch here asks for more
constexpr int BD_ADJ_TILE_H = 32, BD_ADJ_TILE_W = 64, BD_ADJ_PER_THREAD = BD_ADJ_TILE_H * BD_ADJ_TILE_W / BD_THREADS;

__host__ __device__ inline int bd_floor_div(int a, int b) {      // b > 0
    const int q = a / b;
    return a % b < 0 ? q - 1 : q;
}

// x (planes, H, W) -> y (planes, Ho, Wo). cv = ov + Sv, ch = oh + Sh: output (i', j') reads rows s i' + cv - a.
// LDS: taps | footprint rows of `rate` phase runs of wq floats each.
template <int MODE>
__global__ __launch_bounds__(BD_THREADS) void blur_decimate_fwd_kernel(
    const float *__restrict__ x, float *__restrict__ y, const float *__restrict__ k, int kv, int kh, int cv, int ch,
    int rate, int H, int W, int Ho, int Wo, int tile_h, int tile_w, int tiles_y, int tiles_x) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int tiles = tiles_y * tiles_x;
    const int plane = blockIdx.x / tiles;
    const int t = blockIdx.x - plane * tiles;
    const int i0 = (t / tiles_x) * tile_h, j0 = (t % tiles_x) * tile_w;
    const int fh = (tile_h - 1) * rate + kv, fw = (tile_w - 1) * rate + kh;
    const int wq = (fw + rate - 1) / rate, rs = wq * rate;
    const int nk = kv * kh;
    float *s_k = smem;
    float *s_in = smem + ((nk + 3) & ~3);
    for (int idx = tid; idx < nk; idx += BD_THREADS) s_k[idx] = k[idx];
    const float *xp = x + (size_t)plane * H * W;
    const int r0 = rate * i0 + cv - (kv - 1), c0 = rate * j0 + ch - (kh - 1);
    for (int idx = tid; idx < fh * fw; idx += BD_THREADS) {
        const int r = idx / fw, l = idx - r * fw;
        const int m = l / rate, q = l - m * rate;
        s_in[r * rs + q * wq + m] = pad_fetch<MODE>(xp, r0 + r, c0 + l, H, W);
    }
    __syncthreads();
    float *yp = y + (size_t)plane * Ho * Wo;
    const int q0 = (kh - 1) % rate, d0 = (kh - 1) / rate;
    for (int idx = tid; idx < tile_h * tile_w; idx += BD_THREADS) {
        const int r = idx / tile_w, c = idx - r * tile_w;
        if (i0 + r < Ho && j0 + c < Wo) {
            float acc = 0.f;
            for (int a = 0; a < kv; ++a) {
                const float *src = s_in + (rate * r + kv - 1 - a) * rs + c;
                float row = 0.f;
                int q = q0, d = d0;                    // footprint column s c + (kh-1-b) = phase q, index c + d
                for (int b = 0; b < kh; ++b) {
                    row = fmaf(s_k[a * kh + b], src[q * wq + d], row);
                    if (q == 0) q = rate - 1, --d;
                    else --q;
                }
                acc += row;
            }
            yp[(size_t)(i0 + r) * Wo + j0 + c] = acc;
        }
    }
}

// g (planes, h, w) -> out (planes, Ho, Wo), out[r,c] = sum over the wraps (mv, mh) of Z[r - pv + mv Hper, c - ph + mh Wper].
// The canvas of replicate / reflect: (pv, ph) the padding, one wrap (0, 0), out = Z. Circular: pv = ph = 0, out the image.
// LDS: taps | the g rows and columns one pass of the tile reaches, gh_max x gw_max.
__global__ __launch_bounds__(BD_THREADS) void blur_decimate_adj_kernel(
    const float *__restrict__ g, float *__restrict__ out, const float *__restrict__ k, int kv, int kh, int cv, int ch,
    int rate, int h, int w, int Ho, int Wo, int pv, int ph, int Hper, int Wper, int mv_lo, int mv_hi, int mh_lo, int mh_hi,
    int tile_h, int tile_w, int tiles_y, int tiles_x, int gh_max, int gw_max) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int tiles = tiles_y * tiles_x;
    const int plane = blockIdx.x / tiles;
    const int t = blockIdx.x - plane * tiles;
    const int i0 = (t / tiles_x) * tile_h, j0 = (t % tiles_x) * tile_w;
    const int nk = kv * kh;
    float *s_k = smem;
    float *s_g = smem + ((nk + 3) & ~3);
    for (int idx = tid; idx < nk; idx += BD_THREADS) s_k[idx] = k[idx];
    const float *gp = g + (size_t)plane * h * w;
    // the canvas rows and columns that hold anything: s i' + cv - a over the measurement and the taps
    const int ev_lo = cv - (kv - 1), ev_hi = rate * (h - 1) + cv, eh_lo = ch - (kh - 1), eh_hi = rate * (w - 1) + ch;
    float acc[BD_ADJ_PER_THREAD];
#pragma unroll
    for (int n = 0; n < BD_ADJ_PER_THREAD; ++n) acc[n] = 0.f;
    for (int mv = mv_lo; mv <= mv_hi; ++mv) {
        const int e0 = i0 - pv + mv * Hper;
        if (e0 + tile_h - 1 < ev_lo || e0 > ev_hi) continue;
        for (int mh = mh_lo; mh <= mh_hi; ++mh) {
            const int f0 = j0 - ph + mh * Wper;
            if (f0 + tile_w - 1 < eh_lo || f0 > eh_hi) continue;
            const int ilo = bd_floor_div(e0 - cv + rate - 1, rate), jlo = bd_floor_div(f0 - ch + rate - 1, rate);
            __syncthreads();                                // the previous pass is consumed (first time: nothing)
            for (int idx = tid; idx < gh_max * gw_max; idx += BD_THREADS) {
                const int r = idx / gw_max, c = idx - r * gw_max;
                const int gi = ilo + r, gj = jlo + c;
                s_g[idx] = (gi >= 0 && gi < h && gj >= 0 && gj < w) ? gp[(size_t)gi * w + gj] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int n = 0; n < BD_ADJ_PER_THREAD; ++n) {
                const int idx = tid + n * BD_THREADS;
                if (idx < tile_h * tile_w) {
                    const int r = idx / tile_w, c = idx - r * tile_w;
                    const int e = e0 + r, f = f0 + c;
                    // taps a = ra, ra + s, ... reach canvas row e from the measurement rows (e + a - cv) / s
                    const int ra = sei_mod(cv - e, rate), rb = sei_mod(ch - f, rate);
                    const int li0 = (e + ra - cv) / rate - ilo, lj0 = (f + rb - ch) / rate - jlo;
                    float sum = 0.f;
                    for (int a = ra, li = li0; a < kv; a += rate, ++li) {
                        const float *src = s_g + li * gw_max + lj0;
                        const float *kr = s_k + a * kh;
                        float row = 0.f;
                        for (int b = rb, lj = 0; b < kh; b += rate, ++lj) row = fmaf(kr[b], src[lj], row);
                        sum += row;
                    }
                    acc[n] += sum;
                }
            }
        }
    }
    float *op = out + (size_t)plane * Ho * Wo;
#pragma unroll
    for (int n = 0; n < BD_ADJ_PER_THREAD; ++n) {
        const int idx = tid + n * BD_THREADS;
        if (idx < tile_h * tile_w) {
            const int r = idx / tile_w, c = idx - r * tile_w;
            if (i0 + r < Ho && j0 + c < Wo) op[(size_t)(i0 + r) * Wo + j0 + c] = acc[n];
        }
    }
}

// What one call does, from its arguments alone (host arithmetic).
struct BdPlan {
    int h, w;                 // the measurement's extents
    int cv, ch;               // phase + the blur's shift S, per axis
    int pv, ph;               // the canvas padding of replicate / reflect (0 circular)
    size_t work;              // floats of the canvas Z (0: no second launch)
};
static int bd_plan(int planes, int H, int W, int kv, int kh, int mode, int rate, int phase_v, int phase_h, int transpose,
                   BdPlan &pl) {
    SEI_REQUIRE(planes > 0 && H > 0 && W > 0 && kv > 0 && kh > 0);
    SEI_REQUIRE(mode == PAD_CIRCULAR || mode == PAD_REPLICATE || mode == PAD_REFLECT);       // (3, valid: not this operator)
    SEI_REQUIRE(rate >= 1 && rate <= BD_MAX_RATE && phase_v >= 0 && phase_v < rate && phase_h >= 0 && phase_h < rate);
    if (kv > BD_MAX_TAPS || kh > BD_MAX_TAPS || H > (1 << 27) || W > (1 << 27)) return SEI_ERR_TOO_LARGE;
    SEI_REQUIRE(phase_v < H && phase_h < W);                                                // at least one kept sample
    int sv, sh;
    if (mode == PAD_CIRCULAR) {
        sv = kv / 2, sh = kh / 2, pl.pv = pl.ph = 0;
    } else {
        blur_pad_axis(kv, sv, pl.pv);
        blur_pad_axis(kh, sh, pl.ph);
    }
    if (mode == PAD_REFLECT) SEI_REQUIRE(pl.pv <= H - 1 && pl.ph <= W - 1);
    pl.h = (H - phase_v + rate - 1) / rate, pl.w = (W - phase_h + rate - 1) / rate;
    pl.cv = phase_v + sv, pl.ch = phase_h + sh;
    pl.work = transpose && mode != PAD_CIRCULAR ? (size_t)planes * (H + 2 * pl.pv) * (W + 2 * pl.ph) : 0;
    // grids: one workgroup per measurement pixel at worst (forward), per 32 x 64 canvas tile (transpose), per 256 pixels (fold)
    const size_t canvas = sei_ceil_div(H + 2 * pl.pv, BD_ADJ_TILE_H) * sei_ceil_div(W + 2 * pl.ph, BD_ADJ_TILE_W);
    if ((size_t)planes * pl.h * pl.w >= ((size_t)1 << 31) || (size_t)planes * canvas >= ((size_t)1 << 31) ||
        sei_ceil_div((size_t)planes * H * W, 256) >= ((size_t)1 << 31))
        return SEI_ERR_TOO_LARGE;
    return 0;
}

// The forward launch: a tile of 16 x 32 measurement pixels, halved -- rows first, down to one, then columns: a row of 32
// keeps each half-wave on consecutive dwords -- until the taps and the de-interleaved footprint fit BD_LDS. One output
// pixel's own footprint is at most 63 x 64 floats beside 63 x 63 taps, so the loop always ends with a tile.
struct BdFwdLaunch {
    int tile_h, tile_w;
    size_t lds;
};
static BdFwdLaunch bd_fwd_launch(int h, int w, int kv, int kh, int rate) {
    BdFwdLaunch l{h < 16 ? h : 16, w < 32 ? w : 32, 0};
    for (;;) {
        const size_t fh = (size_t)(l.tile_h - 1) * rate + kv, fw = (size_t)(l.tile_w - 1) * rate + kh;
        l.lds = sizeof(float) * ((((size_t)kv * kh + 3) & ~(size_t)3) + fh * (sei_ceil_div(fw, rate) * rate));
        if (l.lds <= BD_LDS) return l;
        if (l.tile_h > 1) l.tile_h = (l.tile_h + 1) / 2;
        else l.tile_w = (l.tile_w + 1) / 2;
    }
}

template <int MODE>
static void bd_fwd(const float *x, float *y, const float *k, int kv, int kh, int planes, int H, int W, int rate,
                   const BdPlan &pl, hipStream_t s) {
    const BdFwdLaunch l = bd_fwd_launch(pl.h, pl.w, kv, kh, rate);
    const int tiles_y = (int)sei_ceil_div(pl.h, l.tile_h), tiles_x = (int)sei_ceil_div(pl.w, l.tile_w);
    const size_t grid = (size_t)planes * tiles_y * tiles_x;
    hipLaunchKernelGGL(blur_decimate_fwd_kernel<MODE>, dim3((unsigned)grid), dim3(BD_THREADS), l.lds, s, x, y, k, kv, kh,
                       pl.cv, pl.ch, rate, H, W, pl.h, pl.w, l.tile_h, l.tile_w, tiles_y, tiles_x);
}

}  // namespace

extern "C" size_t sei_blur_decimate_work_floats(int planes, int H, int W, int kv, int kh, int mode, int rate,
                                                int transpose) {
    BdPlan pl;
    return bd_plan(planes, H, W, kv, kh, mode, rate, 0, 0, transpose, pl) == 0 ? pl.work : 0;
}

extern "C" int sei_blur_decimate(const float *x, float *y, const float *k, int kv, int kh, int planes, int H, int W,
                                 int mode, int rate, int phase_v, int phase_h, int transpose, float *work, void *stream) {
    SEI_REQUIRE(x && y && k);
    BdPlan pl;
    const int rc = bd_plan(planes, H, W, kv, kh, mode, rate, phase_v, phase_h, transpose, pl);
    if (rc != 0) return rc;
    SEI_REQUIRE(pl.work == 0 || work);
    const size_t image = (size_t)planes * H * W, meas = (size_t)planes * pl.h * pl.w;
    const size_t nx = transpose ? meas : image, ny = transpose ? image : meas, nk = (size_t)kv * kh;
    SEI_REQUIRE(!floats_overlap(x, nx, y, ny) && !floats_overlap(k, nk, y, ny));
    if (pl.work) SEI_REQUIRE(!floats_overlap(x, nx, work, pl.work) && !floats_overlap(y, ny, work, pl.work) &&
                             !floats_overlap(k, nk, work, pl.work));
    hipStream_t s = (hipStream_t)stream;
    if (!transpose) {
        switch (mode) {
        case PAD_CIRCULAR: bd_fwd<PAD_CIRCULAR>(x, y, k, kv, kh, planes, H, W, rate, pl, s); break;
        case PAD_REPLICATE: bd_fwd<PAD_REPLICATE>(x, y, k, kv, kh, planes, H, W, rate, pl, s); break;
        default: bd_fwd<PAD_REFLECT>(x, y, k, kv, kh, planes, H, W, rate, pl, s); break;
        }
        return sei_launch_status();
    }
    // the gather writes the canvas (replicate / reflect) or, folding the wraps itself, the image (circular)
    const int Ho = H + 2 * pl.pv, Wo = W + 2 * pl.ph;
    const int tile_h = Ho < BD_ADJ_TILE_H ? Ho : BD_ADJ_TILE_H, tile_w = Wo < BD_ADJ_TILE_W ? Wo : BD_ADJ_TILE_W;
    const int tiles_y = (int)sei_ceil_div(Ho, tile_h), tiles_x = (int)sei_ceil_div(Wo, tile_w);
    const int gh_max = (tile_h + kv - 2) / rate + 1, gw_max = (tile_w + kh - 2) / rate + 1;
    // <= 3972 + 94 * 126 floats (rate 1, 63 x 63 taps): 63,264 bytes
    const size_t lds = sizeof(float) * ((((size_t)kv * kh + 3) & ~(size_t)3) + (size_t)gh_max * gw_max);
    if (lds > BD_LDS) return SEI_ERR_TOO_LARGE;
    int mv_lo = 0, mv_hi = 0, mh_lo = 0, mh_hi = 0;
    if (mode == PAD_CIRCULAR) {
        mv_lo = bd_floor_div(pl.cv - (kv - 1), H), mv_hi = bd_floor_div(rate * (pl.h - 1) + pl.cv, H);
        mh_lo = bd_floor_div(pl.ch - (kh - 1), W), mh_hi = bd_floor_div(rate * (pl.w - 1) + pl.ch, W);
    }
    const size_t grid = (size_t)planes * tiles_y * tiles_x;
    hipLaunchKernelGGL(blur_decimate_adj_kernel, dim3((unsigned)grid), dim3(BD_THREADS), lds, s, x, pl.work ? work : y, k, kv,
                       kh, pl.cv, pl.ch, rate, pl.h, pl.w, Ho, Wo, pl.pv, pl.ph, H, W, mv_lo, mv_hi, mh_lo, mh_hi, tile_h,
                       tile_w, tiles_y, tiles_x, gh_max, gw_max);
    const int status = sei_launch_status();
    if (status != 0 || !pl.work) return status;
    return sei_blur_pad_fold_launch(mode, work, y, planes, H, W, pl.pv, pl.ph, s);
}
