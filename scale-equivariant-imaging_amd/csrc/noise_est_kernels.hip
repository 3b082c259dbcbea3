// Noise-level estimation from measurements alone (noise_estimation.py; the project's own definition, include/sei_hip.h has
// it in full) for gfx950. A is a blur or an antialiased downsampling, so the diagonal Haar detail
// t = ((a - b) - (c - d)) / 2 of a 2 x 2 quad of y is almost pure noise with the variance of a pixel, and the quad's mean s
// says at which intensity. Two kernels:
//
//   noise_quad_hist_kernel : one streaming pass over y. Every workgroup keeps a private 64 x 256 histogram of 32-bit counters
//                            in LDS (64 KiB), adds its quads there with LDS atomics and at the end adds its non-zero bins
//                            to the 64-bit histogram in device memory with global atomics. The counts are integers: the
//                            result does not depend on the order of the atomics. The grid is at most ONE workgroup of 1024
//                            threads per CU: on a noisy image every workgroup ends with a few thousand non-zero bins, and
//                            the global atomics of that flush, not the pass over y, are what the kernel waits for (two
//                            workgroups of 512 per CU: 28.3 us on 3 x 1356 x 2040; one of 512: 20.8; one of 1024: 17.9;
//                            DESIGN 4.20). Threads are laid out as
//                            RW rows x CW columns (powers of two, RW * CW = THREADS) over (row pair, column group), so no thread
//                            divides inside the loop; VEC: a 2 x 4 patch per thread (one float4 per row, two quads), which needs
//                            W % 4 == 0 and a 16-byte aligned base; otherwise one quad per thread from four scalar loads.
//                            Equal bins in consecutive lanes (flat image regions send a whole wave to one counter) are
//                            combined before the atomic: the first lane of a run adds the run's length.
//   noise_fit_kernel       : one workgroup. The integer row and column sums in parallel, then the fit in double precision,
//                            sequential loops in index order, by one thread.
//
// 32-bit LDS counters: a launch covers at most 2^31 quads (the entry point splits the planes into chunks of that many, a
// plane has fewer than 2^28), so no counter of any workgroup can pass 2^31.
#include "sei_common.h"

namespace {

constexpr int THREADS = 1024;
constexpr int LEVELS = 64, BINS = 256, CELLS = LEVELS * BINS;
constexpr unsigned MAX_GRID = 256;                       // one workgroup on each of 256 CUs
constexpr unsigned NO_BIN = 0xFFFFFFFFu;

// the cell of one quad (a b / c d), or NO_BIN when a pixel is outside (0, 1) or not finite
__device__ __forceinline__ unsigned quad_cell(float a, float b, float c, float d) {
    const bool ok = a > 0.f && a < 1.f && b > 0.f && b < 1.f && c > 0.f && c < 1.f && d > 0.f && d < 1.f;
    const float s = __fmul_rn(__fadd_rn(__fadd_rn(a, b), __fadd_rn(c, d)), 0.25f);
    const float t = __fmul_rn(__fsub_rn(__fsub_rn(a, b), __fsub_rn(c, d)), 0.5f);
    if (!ok) return NO_BIN;
    const int l = min(max((int)floorf(__fmul_rn(s, 64.f)), 0), LEVELS - 1);
    const int k = min(BINS - 1, (int)floorf(__fadd_rn(__fmul_rn(fabsf(t), 510.f), 0.5f)));
    return (unsigned)(l * BINS + k);
}

// One LDS atomic per run of equal cells in consecutive lanes. Every lane of the wave calls this (cell = NO_BIN: nothing
// to add).
__device__ __forceinline__ void add_combined(unsigned *h, unsigned cell) {
    const int lane = threadIdx.x & 63;
    const unsigned prev = __shfl_up(cell, 1, 64);
    const bool first = lane == 0 || cell != prev;
    const unsigned long long firsts = __ballot(first);
    if (first && cell != NO_BIN) {
        const unsigned long long above = lane == 63 ? 0ull : firsts >> (lane + 1);
        const unsigned run = above ? (unsigned)__ffsll((long long)above) : (unsigned)(64 - lane);
        atomicAdd(&h[cell], run);
    }
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void noise_quad_hist_kernel(
    const float *__restrict__ y, size_t row_pairs, int H, int W, int H2, int groups, int cw_log2, size_t stride_planes,
    int stride_rows, unsigned long long *__restrict__ hist) {
    __shared__ unsigned h[CELLS];
    for (int i = threadIdx.x; i < CELLS; i += THREADS) h[i] = 0u;
    __syncthreads();

    const int CW = 1 << cw_log2, RW = THREADS >> cw_log2;
    const int tr = threadIdx.x >> cw_log2, tc = threadIdx.x & (CW - 1);
    const size_t first_pair = (size_t)blockIdx.x * RW + tr;
    size_t p = first_pair / H2;                              // plane and row pair of this thread's first item
    int r = (int)(first_pair - p * H2);
    const size_t plane = (size_t)H * W;
    // (the loops are uniform over the workgroup: every lane reaches the shuffles of add_combined)
    for (size_t base = (size_t)blockIdx.x * RW; base < row_pairs; base += (size_t)gridDim.x * RW) {
        const bool row_ok = base + tr < row_pairs;
        const float *top = y + p * plane + (size_t)(2 * r) * W;
        for (int c0 = 0; c0 < groups; c0 += CW) {
            const int c = c0 + tc;
            const bool ok = row_ok && c < groups;
            if (VEC) {
                unsigned cell0 = NO_BIN, cell1 = NO_BIN;
                if (ok) {
                    const float4 u = *reinterpret_cast<const float4 *>(top + 4 * (size_t)c);
                    const float4 v = *reinterpret_cast<const float4 *>(top + W + 4 * (size_t)c);
                    cell0 = quad_cell(u.x, u.y, v.x, v.y);
                    cell1 = quad_cell(u.z, u.w, v.z, v.w);
                }
                add_combined(h, cell0);
                add_combined(h, cell1);
            } else {
                unsigned cell = NO_BIN;
                if (ok) {
                    const float *q = top + 2 * (size_t)c;
                    cell = quad_cell(q[0], q[1], q[W], q[W + 1]);
                }
                add_combined(h, cell);
            }
        }
        p += stride_planes;                                  // the next item: gridDim.x * RW row pairs on
        r += stride_rows;
        if (r >= H2) {
            r -= H2;
            ++p;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CELLS; i += THREADS) {
        const unsigned v = h[i];
        if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
}

__global__ __launch_bounds__(256) void noise_hist_zero_kernel(unsigned long long *__restrict__ hist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < CELLS) hist[i] = 0ull;
}

constexpr double MAD_TO_SIGMA = 0.6744897501960817;      // the median of |N(0, 1)|
constexpr double LATTICE = 510.0;
constexpr int LEVEL_LO = 6, LEVEL_HI = 57;
constexpr unsigned long long N_MIN = 256;

// Interpolated median of a BINS-bin row (stride 1) with total n > 0, in units of the signal; *bin: the median's bin.
__device__ double row_median(const unsigned long long *h, unsigned long long n, int *bin) {
    const double half = (double)n / 2.0;
    unsigned long long below = 0;
    int j = 0;
    for (; j < BINS - 1; ++j) {
        if ((double)(below + h[j]) >= half) break;
        below += h[j];
    }
    *bin = j;
    const double lo = fmax((double)j - 0.5, 0.0), hi = (double)j + 0.5;
    return (lo + (hi - lo) * (half - (double)below) / (double)h[j]) / LATTICE;
}

// The column sums (pooled row) and the row sums n_l are integer sums: the 256 threads take a column each, order does not
// matter. Everything in double precision is thread 0's, sequential and in index order.
__global__ __launch_bounds__(BINS) void noise_fit_kernel(const unsigned long long *__restrict__ hist, double *__restrict__ out) {
    __shared__ unsigned long long pooled[BINS], level_n[LEVELS];
    __shared__ double level_w[LEVELS], level_v[LEVELS];
    const int k = threadIdx.x;
    if (k < LEVELS) level_n[k] = 0ull;
    __syncthreads();
    unsigned long long col = 0;
    for (int l = 0; l < LEVELS; ++l) {
        const unsigned long long c = hist[l * BINS + k];
        col += c;
        unsigned long long row = c;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) row += __shfl_down(row, off, 64);
        if ((k & 63) == 0 && row) atomicAdd(&level_n[l], row);
    }
    pooled[k] = col;
    __syncthreads();
    if (k != 0) return;

    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    unsigned long long n = 0;
    for (int l = 0; l < LEVELS; ++l) n += level_n[l];
    out[6] = 0.0;
    out[7] = 0.0;
    if (n == 0) {
        out[0] = nan; out[1] = nan; out[2] = nan; out[3] = 0.0; out[4] = 0.0; out[5] = 1.0;
        return;
    }
    int flags = 0, bin;
    double sigma = row_median(pooled, n, &bin) / MAD_TO_SIGMA;
    if (bin == BINS - 1) {
        sigma = nan;
        flags |= 2;
    }
    // the used levels: weight n_l and variance v_l (weight 0 = not used)
    double sw = 0.0, swm = 0.0, swv = 0.0, swmm = 0.0, swmv = 0.0;
    int used = 0;
    for (int l = LEVEL_LO; l <= LEVEL_HI; ++l) {
        level_w[l] = 0.0;
        const unsigned long long nl = level_n[l];
        if (nl < N_MIN) continue;
        const double q = row_median(hist + l * BINS, nl, &bin) / MAD_TO_SIGMA;
        if (bin == BINS - 1) continue;
        const double w = (double)nl, m = ((double)l + 0.5) / 64.0, v = q * q;
        level_w[l] = w;
        level_v[l] = v;
        sw += w;
        swm += w * m;
        swv += w * v;
        swmm += w * m * m;
        swmv += w * m * v;
        ++used;
    }
    double eta, gamma, cmm = 0.0, cmv = 0.0, mbar = 0.0, vbar = 0.0;
    if (used >= 2) {                                         // the centred sums of the weighted least-squares line
        mbar = swm / sw;
        vbar = swv / sw;
        for (int l = LEVEL_LO; l <= LEVEL_HI; ++l) {
            const double w = level_w[l];
            if (w == 0.0) continue;
            const double dm = ((double)l + 0.5) / 64.0 - mbar, dv = level_v[l] - vbar;
            cmm += w * dm * dm;
            cmv += w * dm * dv;
        }
    }
    if (used < 2 || !(cmm > 0.0)) {
        gamma = 0.0;
        eta = sigma * sigma;
        flags |= 4;
    } else {
        gamma = cmv / cmm;
        eta = vbar - gamma * mbar;
        if (gamma < 0.0) {
            gamma = 0.0;
            eta = vbar;
            flags |= 8;
        } else if (eta < 0.0) {
            eta = 0.0;
            gamma = swmv / swmm;
            flags |= 16;
        }
    }
    out[0] = sigma; out[1] = eta; out[2] = gamma; out[3] = (double)used; out[4] = (double)n; out[5] = (double)flags;
}

int ceil_log2(int v) {
    int e = 0;
    while ((1 << e) < v) ++e;
    return e;
}

}  // namespace

extern "C" int sei_noise_quad_hist(const float *y, int planes, int H, int W, unsigned long long *hist, int accumulate,
                                   void *stream) {
    SEI_REQUIRE(y && hist);
    SEI_REQUIRE(planes > 0 && H >= 2 && W >= 2 && (size_t)H * W < ((size_t)1 << 30));
    hipStream_t s = (hipStream_t)stream;
    if (!accumulate) hipLaunchKernelGGL(noise_hist_zero_kernel, dim3(CELLS / 256), dim3(256), 0, s, hist);
    const bool vec = W % 4 == 0 && ((uintptr_t)y & 15) == 0;
    const int H2 = H / 2, groups = vec ? W / 4 : W / 2;
    int cw_log2 = ceil_log2(groups);
    if ((1 << cw_log2) > THREADS) cw_log2 = ceil_log2(THREADS);
    const int RW = THREADS >> cw_log2;
    // at most 2^31 quads per launch: the 32-bit counters of a workgroup's LDS histogram cannot overflow
    const size_t quads_per_plane = (size_t)H2 * (W / 2);
    const size_t chunk = ((size_t)1 << 31) / quads_per_plane;        // >= 8: a plane has fewer than 2^28 quads
    for (size_t p0 = 0; p0 < (size_t)planes; p0 += chunk) {
        const size_t np = (size_t)planes - p0 < chunk ? (size_t)planes - p0 : chunk;
        const size_t row_pairs = np * H2;
        const unsigned grid = sei_capped_grid(row_pairs, RW, MAX_GRID);
        const size_t stride = (size_t)grid * RW;
        const float *yp = y + p0 * (size_t)H * W;                   // (a whole number of planes: the alignment of y holds)
        if (vec)
            hipLaunchKernelGGL(noise_quad_hist_kernel<true>, dim3(grid), dim3(THREADS), 0, s, yp, row_pairs, H, W, H2, groups,
                               cw_log2, stride / H2, (int)(stride % H2), hist);
        else
            hipLaunchKernelGGL(noise_quad_hist_kernel<false>, dim3(grid), dim3(THREADS), 0, s, yp, row_pairs, H, W, H2,
                               groups, cw_log2, stride / H2, (int)(stride % H2), hist);
    }
    return sei_launch_status();
}

extern "C" int sei_noise_fit(const unsigned long long *hist, double *out8, void *stream) {
    SEI_REQUIRE(hist && out8);
    hipLaunchKernelGGL(noise_fit_kernel, dim3(1), dim3(BINS), 0, (hipStream_t)stream, hist, out8);
    return sei_launch_status();
}
