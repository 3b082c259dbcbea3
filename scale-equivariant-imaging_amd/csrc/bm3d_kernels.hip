// The two kernels of a BM3D stage for gfx950 (models/bm3d.py documents the algorithm; tests/bm3d_ref.py is its float64
// restatement): block matching, and collaborative filtering of the matched groups (hard thresholding or Wiener) with
// aggregation. All planes of a batch go through one launch per kernel.
//
//   bm3d_match_kernel : one workgroup (256 threads) per reference block. It stages the block's search region, (window + 7)^2
//       floats with zeros outside the image (46 x 46 = 8.3 KiB at window 39), computes d = sum(diff^2) / 64 for every
//       candidate position of the window that lies in the image (thread per candidate; consecutive lanes read consecutive
//       LDS words, the reference block's word is a broadcast), and keeps d where d <= tau, +inf elsewhere. Selection: the
//       key of a candidate is (bits of d) << 32 | (index in the window, row-major); d >= 0, so unsigned order of the keys is
//       the order (d, r', c'). n_max passes, each the minimum over the workgroup (wave shuffles, then one 64-bit LDS
//       atomicMin per wave); the owner of the winner retires it. A minimum is a function of the set of keys: the same bits on
//       every run. The count is cut to the largest power of two not above it; unused slots hold the reference position.
//   bm3d_filter_kernel<WIENER> : one workgroup per tile of 4 x 4 reference blocks of one plane, one group at a time with all
//       256 threads: gather (positions clamped to [0, H-8] x [0, W-8], the count to a power of two in [1, n_max], whatever
//       the index buffer holds), 8-point DCT along the rows and the columns of every block (thread per row / column, in
//       place), Haar along the group (butterflies (a + b) / sqrt 2, (a - b) / sqrt 2 at strides 1, 2, 4 ..., in place: the
//       sums of stride s sit at the multiples of 2s), shrinkage, the group weight by the library's block sum, the inverse
//       transforms, and num += w K block, den += w K with K the outer product of kaiser(8, 2.0).
//       Aggregation, agg = 0: the sums go to an LDS image of the tile's footprint first (LDS float atomics), the tile's
//       (T - 1) step + 8 pixels plus `halo` on every side, 55 x 55 x 2 floats at step 3 and halo 19; the footprint is then
//       added to the global num / den with one float atomic per touched pixel. A block that does not lie inside the footprint
//       (possible only with positions that did not come from bm3d_match_kernel with this window) goes to global memory
//       directly. agg = 1: every block goes to global memory directly (8-float segments). Float atomics in both forms: the
//       stage output is reproducible to rounding, not to the bit.
//   bm3d_finish_kernel : out = num / den (0 where den is 0, which valid groups never leave: the last position of each axis
//       is a reference position and a group always holds its own reference block).
//
// -ffp-contract=off: the float32 operations as written.
#include <limits.h>
#include <math.h>

#include "sei_common.h"

namespace {

constexpr int THREADS = 256, MAX_GROUP = 32, TILE = 4;
constexpr size_t LDS_LIMIT = 64 * 1024;
constexpr double RSQRT2 = 0.70710678118654752440;

// orthonormal DCT-II: DCT8[j * 8 + m] = c_j cos(pi (2 m + 1) j / 16), c_0 = sqrt(1 / 8), c_j = sqrt(2 / 8)
__device__ const float DCT8[64] = {
    0.353553391f, 0.353553391f,  0.353553391f,  0.353553391f,  0.353553391f,  0.353553391f,  0.353553391f,  0.353553391f,
    0.49039264f,  0.415734806f,  0.277785117f,  0.097545161f,  -0.097545161f, -0.277785117f, -0.415734806f, -0.49039264f,
    0.461939766f, 0.191341716f,  -0.191341716f, -0.461939766f, -0.461939766f, -0.191341716f, 0.191341716f,  0.461939766f,
    0.415734806f, -0.097545161f, -0.49039264f,  -0.277785117f, 0.277785117f,  0.49039264f,   0.097545161f,  -0.415734806f,
    0.353553391f, -0.353553391f, -0.353553391f, 0.353553391f,  0.353553391f,  -0.353553391f, -0.353553391f, 0.353553391f,
    0.277785117f, -0.49039264f,  0.097545161f,  0.415734806f,  -0.415734806f, -0.097545161f, 0.49039264f,   -0.277785117f,
    0.191341716f, -0.461939766f, 0.461939766f,  -0.191341716f, -0.191341716f, 0.461939766f,  -0.461939766f, 0.191341716f,
    0.097545161f, -0.277785117f, 0.415734806f,  -0.49039264f,  0.49039264f,   -0.415734806f, 0.277785117f,  -0.097545161f};
// the same table in double, for the hard-thresholding stage (its decisions are taken in double)
__device__ const double DCT8D[64] = {
    0.35355339059327373, 0.35355339059327373, 0.35355339059327373, 0.35355339059327373, 0.35355339059327373, 0.35355339059327373, 0.35355339059327373, 0.35355339059327373,
    0.49039264020161522, 0.41573480615127262, 0.27778511650980114, 0.097545161008064166, -0.097545161008064096, -0.27778511650980098, -0.41573480615127267, -0.49039264020161522,
    0.46193976625564337, 0.19134171618254492, -0.19134171618254486, -0.46193976625564337, -0.46193976625564342, -0.19134171618254517, 0.191341716182545, 0.46193976625564326,
    0.41573480615127262, -0.097545161008064096, -0.49039264020161522, -0.27778511650980109, 0.27778511650980092, 0.49039264020161533, 0.097545161008063958, -0.41573480615127212,
    0.35355339059327379, -0.35355339059327373, -0.35355339059327384, 0.35355339059327368, 0.35355339059327384, -0.35355339059327334, -0.35355339059327356, 0.35355339059327329,
    0.27778511650980114, -0.49039264020161522, 0.097545161008064152, 0.41573480615127273, -0.41573480615127256, -0.097545161008064887, 0.49039264020161516, -0.27778511650980076,
    0.19134171618254492, -0.46193976625564342, 0.46193976625564326, -0.19134171618254495, -0.19134171618254528, 0.4619397662556437, -0.46193976625564354, 0.19134171618254314,
    0.097545161008064166, -0.27778511650980109, 0.41573480615127273, -0.49039264020161533, 0.49039264020161522, -0.41573480615127201, 0.2777851165098022, -0.097545161008062542};
template <typename T>
__device__ __forceinline__ T dct_entry(int i);
template <>
__device__ __forceinline__ float dct_entry<float>(int i) { return DCT8[i]; }
template <>
__device__ __forceinline__ double dct_entry<double>(int i) { return DCT8D[i]; }
// numpy.kaiser(8, 2.0)
__device__ const float KAISER8[8] = {0.43867628f,  0.681324263f, 0.876839905f, 0.985822506f,
                                     0.985822506f, 0.876839905f, 0.681324263f, 0.43867628f};

// position `i` of the reference grid along an axis of extent m: 0, step, 2 step ... and m - 8 last
__host__ __device__ inline int ref_position(int i, int m, int step) {
    const long long p = (long long)i * step;
    return p < m - 8 ? (int)p : m - 8;
}
inline int ref_count(int m, int step) { return (m - 8) / step + 1 + ((m - 8) % step != 0 ? 1 : 0); }

__global__ __launch_bounds__(THREADS) void bm3d_match_kernel(const float *__restrict__ img, int H, int W, int step,
                                                             int window, int nr, int nc, float tau, int n_max,
                                                             int *__restrict__ pos, int *__restrict__ counts,
                                                             float *__restrict__ dist) {
    extern __shared__ unsigned long long match_lds[];
    unsigned long long *best = match_lds;                          // [MAX_GROUP]
    float *region = (float *)(match_lds + MAX_GROUP);              // [RS * RS]
    const int half = window / 2, RS = window + 7, nwin = window * window, nref = nr * nc;
    float *d = region + RS * RS;                                   // [nwin]
    const int tid = (int)threadIdx.x;
    const int plane = (int)(blockIdx.x / (unsigned)nref), ref = (int)(blockIdx.x - (unsigned)plane * (unsigned)nref);
    const int ir = ref / nc, ic = ref - ir * nc;
    const int r = ref_position(ir, H, step), c = ref_position(ic, W, step);
    const float *p = img + (size_t)plane * H * W;
    const int r0 = r - half, c0 = c - half;

    for (int e = tid; e < RS * RS; e += THREADS) {
        const int y = e / RS, x = e - y * RS, gy = r0 + y, gx = c0 + x;
        region[e] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? p[(size_t)gy * W + gx] : 0.f;
    }
    if (tid < MAX_GROUP) best[tid] = ~0ull;
    __syncthreads();

    for (int idx = tid; idx < nwin; idx += THREADS) {
        const int dr = idx / window, dc = idx - dr * window, rr = r0 + dr, cc = c0 + dc;
        float v = INFINITY;
        if (rr >= 0 && rr <= H - 8 && cc >= 0 && cc <= W - 8) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float diff = region[(dr + i) * RS + dc + j] - region[(half + i) * RS + half + j];
                    s += diff * diff;
                }
            s *= 0.015625f;
            v = s <= tau ? s : INFINITY;
        }
        d[idx] = v;
    }
    // (a thread scans only the entries it wrote itself, idx = tid mod THREADS: no barrier needed here)
    int found = 0;
    for (int k = 0; k < n_max; ++k) {
        unsigned long long local = ~0ull;
        for (int idx = tid; idx < nwin; idx += THREADS) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(d[idx]) << 32) | (unsigned)idx;
            local = key < local ? key : local;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned hi = (unsigned)__shfl_xor((int)(local >> 32), off, 64);
            const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)local, off, 64);
            const unsigned long long other = ((unsigned long long)hi << 32) | lo;
            local = other < local ? other : local;
        }
        if ((tid & 63) == 0) atomicMin(&best[k], local);
        __syncthreads();
        const unsigned long long b = best[k];
        if ((unsigned)(b >> 32) >= 0x7f800000u) break;             // nothing under tau is left (the same in every thread)
        const int widx = (int)(unsigned)b;
        if ((widx % THREADS) == tid) d[widx] = INFINITY;           // its owner retires the winner
        ++found;
    }
    __syncthreads();
    int count = 1;
    while (count * 2 <= found) count *= 2;
    const size_t g = (size_t)plane * nref + ref;
    if (tid < n_max) {
        int pr = r, pc = c;
        float pd = INFINITY;
        if (tid < count && tid < found) {
            const unsigned long long b = best[tid];
            const int widx = (int)(unsigned)b;
            pr = r0 + widx / window;
            pc = c0 + widx % window;
            pd = __uint_as_float((unsigned)(b >> 32));
        }
        pos[(g * n_max + tid) * 2] = pr;
        pos[(g * n_max + tid) * 2 + 1] = pc;
        if (dist) dist[g * n_max + tid] = pd;
    }
    if (tid == 0) counts[g] = count;
}

// y[j] = sum_m DCT8[j][m] x[m] (forward) or x[m] = sum_j DCT8[j][m] y[j] (inverse) on 8 LDS words `stride` apart
template <bool INVERSE, typename T>
__device__ __forceinline__ void dct8_lds(T *a, int stride) {
    T x[8], y[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) x[m] = a[m * stride];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        T s = 0;
#pragma unroll
        for (int m = 0; m < 8; ++m) s += dct_entry<T>(INVERSE ? m * 8 + j : j * 8 + m) * x[m];
        y[j] = s;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j * stride] = y[j];
}

// the 2-D DCT of each of the N blocks of A[N][64], in place (one thread per row, then one per column; N * 8 <= THREADS)
template <bool INVERSE, typename T>
__device__ __forceinline__ void dct_blocks(T *A, int N, int tid) {
    if (INVERSE) {
        if (tid < N * 8) dct8_lds<true, T>(A + (tid >> 3) * 64 + (tid & 7), 8);
        __syncthreads();
        if (tid < N * 8) dct8_lds<true, T>(A + tid * 8, 1);
        __syncthreads();
    } else {
        if (tid < N * 8) dct8_lds<false, T>(A + tid * 8, 1);
        __syncthreads();
        if (tid < N * 8) dct8_lds<false, T>(A + (tid >> 3) * 64 + (tid & 7), 8);
        __syncthreads();
    }
}

// one level of the Haar butterflies at stride s along the group, in place
template <typename T>
__device__ __forceinline__ void haar_level(T *A, int N, int s, int tid) {
    const int pairs = (N / (2 * s)) * 64;
    for (int e = tid; e < pairs; e += THREADS) {
        const int i0 = (e >> 6) * 2 * s * 64 + (e & 63), i1 = i0 + s * 64;
        const T a = A[i0], b = A[i1];
        A[i0] = (a + b) * (T)RSQRT2;
        A[i1] = (a - b) * (T)RSQRT2;
    }
    __syncthreads();
}

// T: the type of the transform scratch -- double for hard thresholding (its keep / drop decisions then agree with a float64
// computation except at ties of about 1e-15), float for Wiener (continuous in its inputs)
template <bool WIENER, typename T>
__global__ __launch_bounds__(THREADS) void bm3d_filter_kernel(
    const float *__restrict__ noisy, const float *__restrict__ pilot, const float *__restrict__ var,
    const int *__restrict__ pos, const int *__restrict__ counts, int H, int W, int step, int nr, int nc, int n_max, int halo,
    int fp, double lambd, float *__restrict__ num, float *__restrict__ den, double *__restrict__ coef) {
    extern __shared__ double filter_lds[];
    T *A = (T *)filter_lds;                                        // [MAX_GROUP][64] the noisy group
    T *P = A + MAX_GROUP * 64;                                     // [MAX_GROUP][64] the pilot's group (Wiener only)
    T *thr = P + (WIENER ? MAX_GROUP * 64 : 0);                    // [64] lambd sqrt(v)
    float *vv = (float *)(thr + 64);                               // [64] coefficient variances of the plane
    int *prow = (int *)(vv + 64), *pcol = prow + MAX_GROUP;        // [MAX_GROUP] each
    float *red = (float *)(pcol + MAX_GROUP);                      // [8]: block-sum scratch, [4] = the group weight
    float *fnum = red + 8, *fden = fnum + fp * fp;                 // [fp][fp] each (fp = 0: no footprint image)

    const int tid = (int)threadIdx.x, nref = nr * nc;
    const int tiles_r = (nr + TILE - 1) / TILE, tiles_c = (nc + TILE - 1) / TILE;
    const int plane = (int)(blockIdx.x / (unsigned)(tiles_r * tiles_c));
    const int tile = (int)(blockIdx.x - (unsigned)plane * (unsigned)(tiles_r * tiles_c));
    const int tr = tile / tiles_c, tc = tile - tr * tiles_c;
    const size_t base = (size_t)plane * H * W;
    const int fr0 = ref_position(tr * TILE, H, step) - halo, fc0 = ref_position(tc * TILE, W, step) - halo;

    if (tid < 64) {
        const float v = var[(size_t)plane * 64 + tid];
        vv[tid] = v;
        thr[tid] = (T)(lambd * sqrt((double)v));
    }
    for (int e = tid; e < 2 * fp * fp; e += THREADS) fnum[e] = 0.f;
    __syncthreads();

    for (int gi = 0; gi < TILE * TILE; ++gi) {
        const int ir = tr * TILE + gi / TILE, ic = tc * TILE + gi % TILE;
        if (ir >= nr || ic >= nc) continue;                        // (the same in every thread)
        const size_t g = (size_t)plane * nref + (size_t)ir * nc + ic;
        int N = counts[g];
        N = N < 1 ? 1 : (N > n_max ? n_max : N);
        N = 1 << (31 - __clz(N));                                  // a power of two in [1, n_max], whatever the buffer holds
        if (tid < N) {
            const int pr = pos[(g * n_max + tid) * 2], pc = pos[(g * n_max + tid) * 2 + 1];
            prow[tid] = pr < 0 ? 0 : (pr > H - 8 ? H - 8 : pr);
            pcol[tid] = pc < 0 ? 0 : (pc > W - 8 ? W - 8 : pc);
        }
        __syncthreads();
        for (int e = tid; e < N * 64; e += THREADS) {
            const int k = e >> 6, t = e & 63;
            const size_t at = base + (size_t)(prow[k] + (t >> 3)) * W + pcol[k] + (t & 7);
            A[e] = (T)noisy[at];
            if (WIENER) P[e] = (T)pilot[at];
        }
        __syncthreads();
        dct_blocks<false, T>(A, N, tid);
        if (WIENER) dct_blocks<false, T>(P, N, tid);
        for (int s = 1; s < N; s <<= 1) {
            haar_level(A, N, s, tid);
            if (WIENER) haar_level(P, N, s, tid);
        }
        if (coef)
            for (int e = tid; e < N * 64; e += THREADS) coef[g * n_max * 64 + e] = (double)A[e];

        float local = 0.f;
        for (int e = tid; e < N * 64; e += THREADS) {
            const float v = vv[e & 63];
            if (WIENER) {
                const float pe = (float)P[e], p2 = pe * pe, q = p2 + v;
                const float wc = q > 0.f ? p2 / q : 0.f;
                A[e] *= (T)wc;
                local += wc * wc * v;
            } else {
                const T cf = A[e];
                const bool keep = (cf < 0 ? -cf : cf) > thr[e & 63];
                A[e] = keep ? cf : (T)0;
                local += keep ? v : 0.f;
            }
        }
        const float total = sei_block_sum<THREADS>(local, red);
        if (tid == 0) red[4] = total > 0.f ? 1.0f / total : 1.0f;
        __syncthreads();
        const float w = red[4];

        for (int s = N >> 1; s >= 1; s >>= 1) haar_level(A, N, s, tid);
        dct_blocks<true, T>(A, N, tid);

        for (int e = tid; e < N * 64; e += THREADS) {
            const int k = e >> 6, i = (e & 63) >> 3, j = e & 7;
            const float wk = w * (KAISER8[i] * KAISER8[j]);
            const float val = wk * (float)A[e];
            const int lr = prow[k] - fr0, lc = pcol[k] - fc0;
            if (lr >= 0 && lr + 8 <= fp && lc >= 0 && lc + 8 <= fp) {
                atomicAdd(&fnum[(lr + i) * fp + lc + j], val);
                atomicAdd(&fden[(lr + i) * fp + lc + j], wk);
            } else {
                const size_t at = base + (size_t)(prow[k] + i) * W + pcol[k] + j;
                atomicAdd(&num[at], val);
                atomicAdd(&den[at], wk);
            }
        }
        __syncthreads();
    }

    for (int e = tid; e < fp * fp; e += THREADS) {
        const int y = e / fp, x = e - y * fp, gy = fr0 + y, gx = fc0 + x;
        const float dn = fden[e];
        if (dn != 0.f && gy >= 0 && gy < H && gx >= 0 && gx < W) {
            atomicAdd(&num[base + (size_t)gy * W + gx], fnum[e]);
            atomicAdd(&den[base + (size_t)gy * W + gx], dn);
        }
    }
}

__global__ __launch_bounds__(THREADS) void bm3d_finish_kernel(const float *__restrict__ work, float *__restrict__ out,
                                                              size_t n) {
    for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * THREADS) {
        const float dn = work[n + i];
        out[i] = dn > 0.f ? work[i] / dn : 0.f;
    }
}

bool n_max_ok(int n) { return n == 1 || n == 2 || n == 4 || n == 8 || n == 16 || n == 32; }

struct Bm3dGeometry {
    int nr, nc;
    size_t nref, n;                              // reference blocks of a plane; floats of all planes
};

// 0 on success, else the SEI_ERR_* code
int bm3d_geometry(int planes, int H, int W, int step, int n_max, Bm3dGeometry &g) {
    if (planes < 1 || H < 8 || W < 8 || step < 1 || !n_max_ok(n_max)) return SEI_ERR_BAD_ARG;
    if (H > (1 << 24) || W > (1 << 24)) return SEI_ERR_TOO_LARGE;
    g.nr = ref_count(H, step);
    g.nc = ref_count(W, step);
    g.nref = (size_t)g.nr * g.nc;
    // one dimension of workgroups, int indices of the groups' slots, size_t pixel offsets
    if (g.nref > (size_t)INT_MAX / 64 / MAX_GROUP / (size_t)planes ||
        (size_t)H * W > (SIZE_MAX / sizeof(float)) / 2 / (size_t)planes)
        return SEI_ERR_TOO_LARGE;
    g.n = (size_t)planes * H * W;
    return 0;
}

bool aligned4(const void *a) { return (uintptr_t)a % sizeof(float) == 0; }

template <bool WIENER, typename T>
int bm3d_filter(const float *noisy, const float *pilot, const float *var, const int *pos, const int *counts, int planes,
                int H, int W, int step, int n_max, int window, double lambd, int agg, float *work, double *coef, void *stream) {
    SEI_REQUIRE(noisy && var && pos && counts && work && (!WIENER || pilot));
    SEI_REQUIRE(aligned4(noisy) && aligned4(pilot) && aligned4(var) && aligned4(pos) && aligned4(counts) && aligned4(work) &&
                (uintptr_t)coef % sizeof(double) == 0);
    SEI_REQUIRE(window >= 1 && window % 2 == 1 && (agg == 0 || agg == 1) && lambd >= 0. && lambd <= 3.0e38);
    Bm3dGeometry g;
    const int rc = bm3d_geometry(planes, H, W, step, n_max, g);
    if (rc != 0) return rc;
    SEI_REQUIRE(work != noisy && work != pilot);
    const int halo = window / 2;
    const long long fp_ll = agg == 0 ? (long long)(TILE - 1) * step + 2LL * halo + 8 : 0;
    // bytes: the scratch A (and P) and the thresholds in T; variances, positions, the reduction's words and the footprint in 4
    const size_t fixed = ((size_t)(WIENER ? 2 : 1) * MAX_GROUP * 64 + 64) * sizeof(T) + (64 + 2 * MAX_GROUP + 8) * sizeof(float);
    if (fp_ll > 4096 || fixed + 2 * (size_t)fp_ll * (size_t)fp_ll * sizeof(float) > LDS_LIMIT) return SEI_ERR_TOO_LARGE;
    const int fp = (int)fp_ll;
    const size_t lds = fixed + 2 * (size_t)fp * fp * sizeof(float);
    const size_t tiles = sei_ceil_div((size_t)g.nr, (size_t)TILE) * sei_ceil_div((size_t)g.nc, (size_t)TILE);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(work, 0, 2 * g.n * sizeof(float), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((bm3d_filter_kernel<WIENER, T>), dim3((unsigned)(tiles * (size_t)planes)), dim3(THREADS), lds, s, noisy,
                       pilot, var, pos, counts, H, W, step, g.nr, g.nc, n_max, halo, fp, lambd, work, work + g.n, coef);
    return sei_launch_status();
}

}  // namespace

extern "C" size_t sei_bm3d_ref_blocks(int H, int W, int step) {
    Bm3dGeometry g;
    if (bm3d_geometry(1, H, W, step, 1, g) != 0) return 0;
    return g.nref;
}

extern "C" int sei_bm3d_match(const float *img, int planes, int H, int W, int step, int window, float tau, int n_max, int *pos,
                              int *counts, float *dist, void *stream) {
    SEI_REQUIRE(img && pos && counts);
    SEI_REQUIRE(aligned4(img) && aligned4(pos) && aligned4(counts) && aligned4(dist));
    SEI_REQUIRE(window >= 1 && window % 2 == 1 && tau >= 0.f && tau <= 3.0e38f);
    Bm3dGeometry g;
    const int rc = bm3d_geometry(planes, H, W, step, n_max, g);
    if (rc != 0) return rc;
    if (window > 4096) return SEI_ERR_TOO_LARGE;
    const size_t rs = (size_t)window + 7;
    const size_t lds = MAX_GROUP * sizeof(unsigned long long) + (rs * rs + (size_t)window * window) * sizeof(float);
    if (lds > LDS_LIMIT) return SEI_ERR_TOO_LARGE;
    hipLaunchKernelGGL(bm3d_match_kernel, dim3((unsigned)(g.nref * (size_t)planes)), dim3(THREADS), lds, (hipStream_t)stream,
                       img, H, W, step, window, g.nr, g.nc, tau, n_max, pos, counts, dist);
    return sei_launch_status();
}

extern "C" int sei_bm3d_ht(const float *noisy, const float *var, const int *pos, const int *counts, int planes, int H, int W,
                           int step, int n_max, int window, double lambd, int agg, float *work, double *coef, void *stream) {
    return bm3d_filter<false, double>(noisy, nullptr, var, pos, counts, planes, H, W, step, n_max, window, lambd, agg, work, coef,
                              stream);
}

extern "C" int sei_bm3d_wiener(const float *noisy, const float *pilot, const float *var, const int *pos, const int *counts,
                               int planes, int H, int W, int step, int n_max, int window, int agg, float *work, void *stream) {
    return bm3d_filter<true, float>(noisy, pilot, var, pos, counts, planes, H, W, step, n_max, window, 0., agg, work, nullptr,
                             stream);
}

extern "C" int sei_bm3d_finish(const float *work, float *out, int planes, int H, int W, void *stream) {
    SEI_REQUIRE(work && out && aligned4(work) && aligned4(out));
    SEI_REQUIRE(planes >= 1 && H >= 8 && W >= 8);
    if ((size_t)H * W > (SIZE_MAX / sizeof(float)) / 2 / (size_t)planes) return SEI_ERR_TOO_LARGE;
    const size_t n = (size_t)planes * H * W;
    SEI_REQUIRE(out != work && out != work + n);
    hipLaunchKernelGGL(bm3d_finish_kernel, dim3(sei_capped_grid(n, THREADS, 2048)), dim3(THREADS), 0, (hipStream_t)stream,
                       work, out, n);
    return sei_launch_status();
}
