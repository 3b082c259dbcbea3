// Tiled inference (tiling.py, test.py --tile) for gfx950: cut one (C, H, W) image into overlapping tiles, and blend the
// tiles a model returned back into one image. The plan of an axis of length n with tile T and overlap v (stride s = T - v)
// is never passed as a list: one tile of extent n at origin 0 where n <= T, otherwise tiles of extent T at the origins
// 0, s, 2s, ... strictly below n - T and a last one at n - T, shifted back to end on the border. Nothing is padded. With
// 2 v <= T at most three tiles of an axis cover a pixel.
//
//   tile_gather_kernel : tiles[t - t0] = x[:, oy : oy + Th, ox : ox + Tw] for the tiles t0 .. t0 + n - 1 (row-major over
//                        the ny x nx grid), a bit-for-bit copy. A thread owns four consecutive floats of one (tile,
//                        channel) plane of the batch.
//   tile_blend_kernel  : out[c, y, x] (+)= sum over the covering tiles of the chunk, in tile order, of wy wx tile[c, y - oy,
//                        x - ox], one fmaf per tile, and with `finish` the quotient by Sy(y) Sx(x), the per-axis weight
//                        sums over ALL tiles of the plan. Gather form: a thread owns four consecutive output pixels of one
//                        row of one channel and finds their tiles arithmetically; no atomics, so chunked calls leave the
//                        bits of one call.
//
// Both kernels work on groups of four floats that sit on the 16-byte grid of the buffer they WRITE (the tile batch, the
// output image): a full group is one 16-byte store, the partial groups at the ends of a row (or of a tile plane) are scalar
// stores. Reads are 16 bytes wide where the four source floats are contiguous and aligned, scalar otherwise. The
// arithmetic per pixel does not depend on which form moved it, so any alignment gives the same bits. Streaming kernels:
// consecutive lanes own consecutive groups, the grid is capped and strided, no LDS.
#include "sei_common.h"

namespace {

constexpr int THREADS = 256;
constexpr unsigned MAX_GRID = 2048;      // 256 CUs x 8 workgroups; the rest of the work is grid-strided
constexpr unsigned MAX_GRID_Y = 65535;
constexpr int MAX_TILE = 2048;           // weights <= 1024, a product <= 2^20, nine of them < 2^24: exact in float32

enum { WINDOW_UNIFORM = 0, WINDOW_FEATHER = 1, WINDOW_CROP = 2 };

// one axis of the plan: image extent n, tile extent T, stride s, tile count k
struct Axis {
    int n, T, s, k;
};

__device__ __forceinline__ int axis_origin(const Axis &a, int i) { return i < a.k - 1 ? i * a.s : a.n - a.T; }

// window weight of image position p under the tile at origin o (0 outside the tile)
__device__ __forceinline__ int axis_weight(const Axis &a, int window, int o, int p) {
    const int i = p - o;
    if (i < 0 || i >= a.T) return 0;
    const int v = a.T - a.s;
    if (window == WINDOW_UNIFORM) return 1;
    if (window == WINDOW_FEATHER) return min(min(i + 1, a.T - i), max(v, 1));
    const int lo = o == 0 ? 0 : v / 2, hi = o + a.T == a.n ? 0 : v - v / 2;
    return i >= lo && i < a.T - hi;
}

// The tiles that can touch the positions [pa, pb], in ascending order: the regular tiles first .. first + count - 2 (origin
// i s, i <= k - 2), then the shifted last tile k - 1. Slot j of `count` names tile axis_slot(...).
__device__ __forceinline__ void axis_candidates(const Axis &a, int pa, int pb, int &first, int &count) {
    const int below = pa - a.T + 1;                       // origins >= below reach pa
    first = below <= 0 ? 0 : (below + a.s - 1) / a.s;
    const int last = min(pb / a.s, a.k - 2);
    count = max(last - first + 1, 0) + 1;
}
__device__ __forceinline__ int axis_slot(const Axis &a, int first, int count, int j) {
    return j < count - 1 ? first + j : a.k - 1;
}

__global__ __launch_bounds__(THREADS) void tile_gather_kernel(const float *__restrict__ x, float *__restrict__ tiles, int C,
                                                              Axis ay, Axis ax, int t0, int planes, int lead0) {
    const unsigned tile_plane = (unsigned)ay.T * ax.T;
    const size_t plane = (size_t)ay.n * ax.n;
    for (int tc = blockIdx.y; tc < planes; tc += gridDim.y) {                  // (tile, channel) planes of the batch
        const int t = t0 + tc / C, c = tc % C;
        const int oy = axis_origin(ay, t / ax.k), ox = axis_origin(ax, t % ax.k);
        const float *src = x + (size_t)c * plane + (size_t)oy * ax.n + ox;
        float *dst = tiles + (size_t)tc * tile_plane;
        const unsigned lead = (unsigned)((lead0 + (size_t)tc * tile_plane) & 3);   // floats of dst past the 16-byte grid
        const unsigned groups = (tile_plane + lead + 3) / 4;
        for (unsigned g = blockIdx.x * THREADS + threadIdx.x; g < groups; g += gridDim.x * THREADS) {
            const unsigned e0 = g == 0 ? 0 : 4 * g - lead, e1 = min(4 * g + 4 - lead, tile_plane);
            const unsigned iy = e0 / ax.T, ix = e0 - iy * ax.T;
            if (e1 - e0 == 4 && ix + 3 < (unsigned)ax.T) {                    // a full group inside one tile row
                const float *s = src + (size_t)iy * ax.n + ix;
                float4 v;
                if (((uintptr_t)s & 15) == 0) {
                    v = *reinterpret_cast<const float4 *>(s);
                } else {
                    v.x = s[0]; v.y = s[1]; v.z = s[2]; v.w = s[3];
                }
                *reinterpret_cast<float4 *>(dst + e0) = v;
            } else {                                                          // across a row end, or at an end of the plane
                for (unsigned e = e0; e < e1; ++e) {
                    const unsigned jy = e / ax.T, jx = e - jy * ax.T;
                    dst[e] = src[(size_t)jy * ax.n + jx];
                }
            }
        }
    }
}

__global__ __launch_bounds__(THREADS) void tile_blend_kernel(const float *__restrict__ tiles, float *__restrict__ out, int C,
                                                             Axis ay, Axis ax, int window, int t0, int n, int accumulate,
                                                             int finish, int lead0) {
    // a row of W pixels that starts up to 3 floats past the 16-byte grid holds at most (W + 3 + 3) / 4 groups
    const unsigned row_groups = (unsigned)(ax.n + 6) / 4;
    const unsigned groups = (unsigned)ay.n * row_groups;                       // < 2^31: H W < 2^30
    const size_t tile_plane = (size_t)ay.T * ax.T, plane = (size_t)ay.n * ax.n;
    for (int c = blockIdx.y; c < C; c += gridDim.y) {
        for (unsigned gi = blockIdx.x * THREADS + threadIdx.x; gi < groups; gi += gridDim.x * THREADS) {
            const int y = (int)(gi / row_groups), g = (int)(gi - (unsigned)y * row_groups);
            float *row = out + (size_t)c * plane + (size_t)y * ax.n;
            const int a = (int)((lead0 + (size_t)c * plane + (size_t)y * ax.n) & 3);   // floats of row past the grid
            const int xa = max(4 * g - a, 0), xb = min(4 * g - a + 3, ax.n - 1);      // pixels [xa, xb] of the row
            if (xa > xb) continue;
            const bool full = xb - xa == 3;

            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            if (accumulate) {
                if (full) {
                    const float4 q = *reinterpret_cast<const float4 *>(row + xa);
                    acc[0] = q.x; acc[1] = q.y; acc[2] = q.z; acc[3] = q.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (xa + j <= xb) acc[j] = row[xa + j];
                }
            }

            int yfirst, ycount, xfirst, xcount;
            axis_candidates(ay, y, y, yfirst, ycount);
            axis_candidates(ax, xa, xb, xfirst, xcount);
            // ascending t = ty nx + tx: rows of tiles in order, and in each its columns in order
            int sum_y = 0;
            for (int jy = 0; jy < ycount; ++jy) {
                const int ty = axis_slot(ay, yfirst, ycount, jy);
                const int oy = axis_origin(ay, ty);
                const int wy = axis_weight(ay, window, oy, y);
                sum_y += wy;
                if (wy == 0) continue;
                for (int jx = 0; jx < xcount; ++jx) {
                    const int tx = axis_slot(ax, xfirst, xcount, jx);
                    const int t = ty * ax.k + tx;
                    if (t < t0 || t >= t0 + n) continue;
                    const int ox = axis_origin(ax, tx);
                    int w[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) w[j] = xa + j <= xb ? wy * axis_weight(ax, window, ox, xa + j) : 0;
                    if ((w[0] | w[1] | w[2] | w[3]) == 0) continue;
                    const float *src = tiles + ((size_t)(t - t0) * C + c) * tile_plane + (size_t)(y - oy) * ax.T;
                    const int i0 = xa - ox;
                    float v[4] = {0.f, 0.f, 0.f, 0.f};
                    if (i0 >= 0 && i0 + 3 < ax.T && ((uintptr_t)(src + i0) & 15) == 0) {
                        const float4 q = *reinterpret_cast<const float4 *>(src + i0);
                        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (w[j] != 0) v[j] = src[i0 + j];
                    }
                    // a tile whose weight is 0 at a pixel is not part of that pixel's sum: its value is not looked at
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (w[j] != 0) acc[j] = fmaf((float)w[j], v[j], acc[j]);
                }
            }

            if (finish) {
                // Sx over every tile of the axis, whichever chunk this call holds
                int sum_x[4] = {0, 0, 0, 0};
                for (int jx = 0; jx < xcount; ++jx) {
                    const int ox = axis_origin(ax, axis_slot(ax, xfirst, xcount, jx));
#pragma unroll
                    for (int j = 0; j < 4; ++j) sum_x[j] += axis_weight(ax, window, ox, xa + j);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (xa + j <= xb) acc[j] = __fdiv_rn(acc[j], (float)(sum_y * sum_x[j]));
            }
            if (full) {
                *reinterpret_cast<float4 *>(row + xa) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (xa + j <= xb) row[xa + j] = acc[j];
            }
        }
    }
}

// one axis is the canonical plan of its image extent: a single tile of the image's extent, or k >= 2 tiles of extent T at
// stride s with 2 (T - s) <= T, the last regular origin strictly below n - T and the one after it not
bool axis_ok(int n, int T, int s, int k) {
    if (n < 1 || T < 1 || s < 1 || k < 1 || T > MAX_TILE || s > T) return false;
    if (k == 1) return T == n;
    if (2 * (T - s) > T) return false;
    const long long gap = (long long)n - T;
    return (long long)(k - 2) * s < gap && gap <= (long long)(k - 1) * s;
}

bool disjoint(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa + a_bytes <= pb || pb + b_bytes <= pa;
}

// the arguments both entry points share
bool plan_ok(const void *image, const void *tiles, int C, int H, int W, int Th, int Tw, int sy, int sx, int ny, int nx,
             int t0, int n) {
    if (!image || !tiles || ((uintptr_t)image & 3) || ((uintptr_t)tiles & 3) || C < 1) return false;
    if (!axis_ok(H, Th, sy, ny) || !axis_ok(W, Tw, sx, nx)) return false;
    if ((size_t)H * W >= ((size_t)1 << 30) || (long long)ny * nx >= (1ll << 31)) return false;
    if (t0 < 0 || n < 1 || (long long)t0 + n > (long long)ny * nx) return false;
    if ((long long)n * C >= (1ll << 31)) return false;                        // a (tile, channel) plane index is an int
    return disjoint(image, (size_t)C * H * W * sizeof(float), tiles, (size_t)n * C * Th * Tw * sizeof(float));
}

}  // namespace

extern "C" int sei_tile_gather(const float *x, float *tiles, int C, int H, int W, int Th, int Tw, int sy, int sx, int ny,
                               int nx, int t0, int n, void *stream) {
    SEI_REQUIRE(plan_ok(x, tiles, C, H, W, Th, Tw, sy, sx, ny, nx, t0, n));
    const int planes = n * C;
    const int lead0 = (int)(((uintptr_t)tiles >> 2) & 3);                     // floats past the 16-byte grid
    const Axis ay{H, Th, sy, ny}, ax{W, Tw, sx, nx};
    const dim3 grid(sei_capped_grid((size_t)Th * Tw / 4 + 2, THREADS, MAX_GRID), sei_capped_grid(planes, 1, MAX_GRID_Y));
    hipLaunchKernelGGL(tile_gather_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, x, tiles, C, ay, ax, t0, planes,
                       lead0);
    return sei_launch_status();
}

extern "C" int sei_tile_blend(const float *tiles, float *out, int C, int H, int W, int Th, int Tw, int sy, int sx, int ny,
                              int nx, int window, int t0, int n, int accumulate, int finish, void *stream) {
    SEI_REQUIRE(window >= WINDOW_UNIFORM && window <= WINDOW_CROP);
    SEI_REQUIRE(plan_ok(out, tiles, C, H, W, Th, Tw, sy, sx, ny, nx, t0, n));
    const int lead0 = (int)(((uintptr_t)out >> 2) & 3);
    const Axis ay{H, Th, sy, ny}, ax{W, Tw, sx, nx};
    const size_t groups = (size_t)H * ((W + 6) / 4);
    const dim3 grid(sei_capped_grid(groups, THREADS, MAX_GRID), sei_capped_grid(C, 1, MAX_GRID_Y));
    hipLaunchKernelGGL(tile_blend_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, tiles, out, C, ay, ax, window, t0, n,
                       accumulate, finish, lead0);
    return sei_launch_status();
}
