// The proximal operator of the isotropic total variation for gfx950: `iters` iterations of the primal-dual loop that
// models/tv.py documents (deepinv v0.2.0's TVDenoiser restated: tau 0.01, sigma 1 / (8 tau), rho 1.99), on the state
// (x2, u2) of `planes` independent H x W planes.
//
//   tv_prox_kernel<T, K, THREADS> : one workgroup per (T x T tile, plane). It stages the tile plus a halo of K pixels
//       (a region of R x R, R = T + 2K), advances it by n <= K iterations on chip, and stores the tile's interior to the
//       OTHER state buffer: neighbouring tiles still read the old one. After iteration t the values of the region's
//       outermost t rings are stale and are never read again: the valid region shrinks by one ring per iteration and
//       ends as the tile. A launch of n < K iterations stages only a halo of n.
//   sei_tv_prox : ceil(iters / K) such launches that alternate between (x2, u2) and `work`; when their number is odd
//       one device-to-device copy brings the state back into (x2, u2).
//
// What lives where. z and x2 of a pixel are read and written by that pixel's thread only, so they stay in REGISTERS for
// the whole launch (each thread owns SLOTS = ceil(R^2 / THREADS) fixed pixels). LDS holds what neighbours read: the two
// dual planes u2v, u2h and w = 2 x - x2 of the current iteration, three arrays of R^2 floats. Consecutive lanes own
// consecutive LDS words (row pitch R, no padding), so every shifted read (left, up, down, right) is a run of consecutive
// words per half-wave: no bank conflict. An iteration is two phases with a barrier after each:
//       A  x from (z, x2, u2 at the pixel, above it and left of it); w -> LDS; x2 <- x2 + rho (x - x2)
//       B  u from (u2 at the pixel, w at the pixel, below it and right of it); u2 <- u2 + rho (u - u2), in place
// LDS per workgroup and residency (160 KiB per CU; THREADS = 1024 at T = 64, 256 at T = 32):
//       T = 64: K = 1, 2, 4, 5 -> 51, 54, 61, 64 KiB: two workgroups (32 waves, the CU's limit) per CU;
//               K = 10 -> 83 KiB, K = 20 -> 127 KiB: one workgroup (16 waves) per CU
//       T = 32: K = 1 .. 10 -> 13 .. 32 KiB: 8 .. 5 workgroups of 4 waves per CU; K = 20 -> 61 KiB: two
// Redundant arithmetic (halo pixels advanced and thrown away) at K = 5: 1.16x at T = 64, 1.35x at T = 32. Measured
// (DESIGN 4.7), T = 32 is nevertheless the faster one on planes of more than one tile; why has not been profiled.
//
// Neumann boundary: a difference across the IMAGE's edge is zero (tv_pixel_x / tv_pixel_u get one flag per neighbour
// that exists in the image). A region's own edge is not a boundary: pixels there are simply not advanced.
//
// The arithmetic of one pixel-iteration is the two functions tv_pixel_x and tv_pixel_u: explicit fmaf, correctly
// rounded division and square root, no contraction (-ffp-contract=off). Their results depend on the operand values
// only, so every tiling, every K and every split of `iters` into calls gives the same bits. No atomics.
#include <limits.h>

#include "sei_common.h"

namespace {

constexpr float TAU = 0.01f, SIGMA = 12.5f, RHO = 1.99f, ONE_PLUS_TAU = 1.01f;

enum : unsigned { IN_IMAGE = 1u << 16, HAS_UP = 1u << 17, HAS_DOWN = 1u << 18, HAS_LEFT = 1u << 19, HAS_RIGHT = 1u << 20 };

// x = (x2 - tau * nabla_adjoint(u2) + tau * z) / (1 + tau); the four operands are u2v above / at and u2h left of / at the
// pixel, already zero where the image has no such difference
__device__ __forceinline__ float tv_pixel_x(float z, float x2, float uv_up, float uv, float uh_left, float uh) {
    const float adj = (uv_up - uv) + (uh_left - uh);
    return __fdiv_rn(fmaf(TAU, z, fmaf(-TAU, adj, x2)), ONE_PLUS_TAU);
}

// v = u2 + sigma * nabla(w); u = v / max(|v|_2 / ths, 1); (dv, dh) = nabla(w) at the pixel, zero across the image's edge
__device__ __forceinline__ void tv_pixel_u(float dv, float dh, float ths, float &u2v, float &u2h) {
    const float vv = fmaf(SIGMA, dv, u2v), vh = fmaf(SIGMA, dh, u2h);
    const float norm = __fsqrt_rn(fmaf(vv, vv, vh * vh));
    const float den = fmaxf(__fdiv_rn(norm, ths), 1.0f);
    const float uv = __fdiv_rn(vv, den), uh = __fdiv_rn(vh, den);
    u2v = fmaf(RHO, uv - u2v, u2v);
    u2h = fmaf(RHO, uh - u2h, u2h);
}

template <int T, int K, int THREADS>
__global__ __launch_bounds__(THREADS) void tv_prox_kernel(const float *__restrict__ z, const float *__restrict__ x2_in,
                                                          const float *__restrict__ u2_in, float *__restrict__ x2_out,
                                                          float *__restrict__ u2_out, int planes, int H, int W,
                                                          int tiles_x, int tiles, float ths, int n) {
    constexpr int R = T + 2 * K, RR = R * R;
    constexpr int SLOTS = (RR + THREADS - 1) / THREADS;
    __shared__ float lds[3 * RR];
    float *UV = lds, *UH = lds + RR, *WW = lds + 2 * RR;

    const int plane = blockIdx.x / tiles, tile = blockIdx.x - plane * tiles;
    const int ty0 = (tile / tiles_x) * T, tx0 = (tile % tiles_x) * T;
    const size_t hw = (size_t)H * W, pv = (size_t)plane * hw, ph = ((size_t)planes + plane) * hw;
    const int skip = K - n;                      // rings of the region this launch does not need: a halo of n suffices

    // per slot: the pixel's row and column in the region (bytes 0 and 1) and which of its neighbours exist in the image
    unsigned meta[SLOTS];
    float zr[SLOTS], xr[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int idx = s * THREADS + (int)threadIdx.x;
        const int r = idx / R, c = idx - r * R;
        const int gi = ty0 - K + r, gj = tx0 - K + c;
        unsigned m = (unsigned)r | ((unsigned)c << 8);
        const bool staged = idx < RR && r >= skip && r < R - skip && c >= skip && c < R - skip;
        float zv = 0.f, xv = 0.f, uv = 0.f, uh = 0.f;
        if (staged && gi >= 0 && gi < H && gj >= 0 && gj < W) {
            m |= IN_IMAGE | (gi >= 1 ? HAS_UP : 0u) | (gi < H - 1 ? HAS_DOWN : 0u) | (gj >= 1 ? HAS_LEFT : 0u) |
                 (gj < W - 1 ? HAS_RIGHT : 0u);
            const size_t p = (size_t)gi * W + gj;
            zv = z[pv + p];
            xv = x2_in[pv + p];
            uv = u2_in[pv + p];
            uh = u2_in[ph + p];
        }
        meta[s] = m;
        zr[s] = zv;
        xr[s] = xv;
        if (idx < RR) {
            UV[idx] = uv;
            UH[idx] = uh;
        }
    }
    __syncthreads();

    for (int t = 1; t <= n; ++t) {
        const int lo = skip + t;                 // phase A advances rows and columns lo .. R - lo, phase B lo .. R - 1 - lo
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const unsigned m = meta[s];
            const int r = m & 0xFF, c = (m >> 8) & 0xFF, idx = s * THREADS + (int)threadIdx.x;
            if ((m & IN_IMAGE) && r >= lo && r <= R - lo && c >= lo && c <= R - lo) {
                const float uv = (m & HAS_DOWN) ? UV[idx] : 0.f, uv_up = (m & HAS_UP) ? UV[idx - R] : 0.f;
                const float uh = (m & HAS_RIGHT) ? UH[idx] : 0.f, uh_left = (m & HAS_LEFT) ? UH[idx - 1] : 0.f;
                const float x2 = xr[s];
                const float x = tv_pixel_x(zr[s], x2, uv_up, uv, uh_left, uh);
                WW[idx] = fmaf(2.0f, x, -x2);
                xr[s] = fmaf(RHO, x - x2, x2);
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const unsigned m = meta[s];
            const int r = m & 0xFF, c = (m >> 8) & 0xFF, idx = s * THREADS + (int)threadIdx.x;
            if ((m & IN_IMAGE) && r >= lo && r < R - lo && c >= lo && c < R - lo) {
                const float w = WW[idx];
                const float dv = (m & HAS_DOWN) ? WW[idx + R] - w : 0.f;
                const float dh = (m & HAS_RIGHT) ? WW[idx + 1] - w : 0.f;
                float uv = UV[idx], uh = UH[idx];
                tv_pixel_u(dv, dh, ths, uv, uh);
                UV[idx] = uv;
                UH[idx] = uh;
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const unsigned m = meta[s];
        const int r = m & 0xFF, c = (m >> 8) & 0xFF, idx = s * THREADS + (int)threadIdx.x;
        if ((m & IN_IMAGE) && r >= K && r < K + T && c >= K && c < K + T) {
            const size_t p = (size_t)(ty0 - K + r) * W + (tx0 - K + c);
            x2_out[pv + p] = xr[s];
            u2_out[pv + p] = UV[idx];
            u2_out[ph + p] = UH[idx];
        }
    }
}

struct TvGeometry {
    int tiles_x, tiles;
    size_t n;                                    // floats of one copy of x2: planes * H * W
};

// 0 on success, else the SEI_ERR_* code
int tv_geometry(int planes, int H, int W, int tile, TvGeometry &g) {
    if (planes < 1 || H < 1 || W < 1) return SEI_ERR_BAD_ARG;
    const size_t tx = sei_ceil_div((size_t)W, (size_t)tile), ty = sei_ceil_div((size_t)H, (size_t)tile);
    const size_t hw = (size_t)H * (size_t)W;
    // the grid is one dimension of tiles * planes workgroups; pixel offsets are size_t, row and column indices int
    if (H > (1 << 30) || W > (1 << 30) || tx * ty > (size_t)INT_MAX / (size_t)planes ||
        hw > (SIZE_MAX / sizeof(float)) / 3 / (size_t)planes)
        return SEI_ERR_TOO_LARGE;
    g.tiles_x = (int)tx;
    g.tiles = (int)(tx * ty);
    g.n = hw * (size_t)planes;
    return 0;
}

bool overlap(const float *a, size_t na, const float *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb * sizeof(float) && b0 < a0 + na * sizeof(float);
}

template <int T, int K>
void tv_launch(const float *z, const float *x2_in, const float *u2_in, float *x2_out, float *u2_out, int planes, int H,
               int W, const TvGeometry &g, float ths, int n, hipStream_t s) {
    constexpr int THREADS = T == 64 ? 1024 : 256;
    hipLaunchKernelGGL((tv_prox_kernel<T, K, THREADS>), dim3((unsigned)g.tiles * (unsigned)planes), dim3(THREADS), 0, s, z,
                       x2_in, u2_in, x2_out, u2_out, planes, H, W, g.tiles_x, g.tiles, ths, n);
}

template <int T>
bool tv_launch_k(int k, const float *z, const float *x2_in, const float *u2_in, float *x2_out, float *u2_out, int planes,
                 int H, int W, const TvGeometry &g, float ths, int n, hipStream_t s) {
    switch (k) {
#define SEI_TV_CASE(KK) \
    case KK: tv_launch<T, KK>(z, x2_in, u2_in, x2_out, u2_out, planes, H, W, g, ths, n, s); return true;
        SEI_TV_CASE(1)
        SEI_TV_CASE(2)
        SEI_TV_CASE(4)
        SEI_TV_CASE(5)
        SEI_TV_CASE(10)
        SEI_TV_CASE(20)
#undef SEI_TV_CASE
    }
    return false;
}

bool tv_k_ok(int k) { return k == 1 || k == 2 || k == 4 || k == 5 || k == 10 || k == 20; }

// The default schedule, from the measured table of DESIGN 4.7: k = 5 everywhere; a plane that fits one 64 x 64 tile
// takes it (one workgroup per plane, no halo to recompute), anything larger runs 32 x 32 tiles.
constexpr int DEFAULT_K = 5, SMALLEST_TILE = 32;
int tv_default_tile(int H, int W) { return H <= 64 && W <= 64 ? 64 : 32; }

}  // namespace

extern "C" size_t sei_tv_prox_work_floats(int planes, int H, int W) {
    TvGeometry g;
    if (tv_geometry(planes, H, W, SMALLEST_TILE, g) != 0) return 0;
    return 3 * g.n;
}

extern "C" int sei_tv_prox_ex(const float *z, float *x2, float *u2, int planes, int H, int W, float ths, int iters,
                              int tile, int k, float *work, void *stream) {
    SEI_REQUIRE(z && x2 && u2 && work);
    SEI_REQUIRE(planes >= 1 && H >= 1 && W >= 1 && iters >= 1 && ths > 0.f);
    SEI_REQUIRE(((uintptr_t)z | (uintptr_t)x2 | (uintptr_t)u2 | (uintptr_t)work) % sizeof(float) == 0);
    if (tile == 0) tile = tv_default_tile(H, W);
    if (k == 0) k = DEFAULT_K;
    SEI_REQUIRE((tile == 32 || tile == 64) && tv_k_ok(k));
    TvGeometry g;
    int rc = tv_geometry(planes, H, W, SMALLEST_TILE, g);        // refuse what sei_tv_prox_work_floats refuses
    if (rc == 0) rc = tv_geometry(planes, H, W, tile, g);
    if (rc != 0) return rc;
    SEI_REQUIRE(!overlap(z, g.n, x2, g.n) && !overlap(z, g.n, u2, 2 * g.n) && !overlap(z, g.n, work, 3 * g.n) &&
                !overlap(x2, g.n, u2, 2 * g.n) && !overlap(x2, g.n, work, 3 * g.n) && !overlap(u2, 2 * g.n, work, 3 * g.n));
    hipStream_t s = (hipStream_t)stream;
    float *wx = work, *wu = work + g.n;
    bool in_work = false;                        // where the current state is
    for (int left = iters; left > 0; left -= k) {
        const int n = left < k ? left : k;
        const float *xi = in_work ? wx : x2, *ui = in_work ? wu : u2;
        float *xo = in_work ? x2 : wx, *uo = in_work ? u2 : wu;
        const bool ok = tile == 64 ? tv_launch_k<64>(k, z, xi, ui, xo, uo, planes, H, W, g, ths, n, s)
                                   : tv_launch_k<32>(k, z, xi, ui, xo, uo, planes, H, W, g, ths, n, s);
        if (!ok) return SEI_ERR_BAD_ARG;
        in_work = !in_work;
    }
    if (in_work) {
        hipError_t e = hipMemcpyAsync(x2, wx, g.n * sizeof(float), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(u2, wu, 2 * g.n * sizeof(float), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return (int)e;
    }
    return sei_launch_status();
}

extern "C" int sei_tv_prox(const float *z, float *x2, float *u2, int planes, int H, int W, float ths, int iters,
                           float *work, void *stream) {
    return sei_tv_prox_ex(z, x2, u2, planes, H, W, ths, iters, 0, 0, work, stream);
}
