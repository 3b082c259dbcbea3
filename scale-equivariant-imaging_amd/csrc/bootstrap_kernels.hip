// Equivariant bootstrap of the evaluation step (bootstrap.py; Tachella and Pereyra, "Equivariant bootstrapping for
// uncertainty quantification in imaging inverse problems", restated from the paper) for gfx950. Per replica r the host
// zooms the reconstruction out (a_r = T_r x), measures it again with fresh noise, reconstructs it (b_r), and these kernels
// do everything around the two operator calls:
//
//   boot_scale_fwd_kernel      : a_r = T_r x for all replicas of a chunk from ONE (C, H, W) image: the padded zoom-out of
//                                physics_kernels.hip (bicubic A = -0.75, reflection, align_corners=True, the grid
//                                (g - c) / rate + c) on a grid that is laid out by rows and columns: x from column j over W,
//                                y from row i over H. sei_scale_resample_fwd keeps the reference's (w, h) meshgrid viewed as
//                                (h, w); the two agree bit for bit where H == W and only there.
//   boot_luma_diff_kernel      : d = Y(q(a)) - Y(q(b)) per pixel, q the 8-bit quantisation and clamp of test.py, Y the luma
//                                of metrics.py, and the per-workgroup sums of d^2; boot_luma_sum_kernel adds an image's
//                                partial sums in index order, in double. No atomics; the grid of an image depends on its
//                                pixel count only, so its sum does not depend on the batch it is in.
//   boot_pullback_accum_kernel : msq[p] (+)= sum_r (T_r^+ d_r)[p]^2, T_r^+ the same gather at rate (g - c) + c, the
//                                replicas in order through one fmaf chain per pixel: chunked calls give one call's bits.
#include "sei_common.h"
#include "bicubic_taps.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_PARTS = 256;       // partial sums per image at the most

// normalised base coordinates of output pixel (i, j): scale_taps' operations with aa = i, bb = j
__device__ __forceinline__ void base_grid(int i, int j, float two_over_h, float two_over_w, float &v, float &u) {
    v = __fsub_rn(__fmul_rn(two_over_w, (float)j), 1.f);       // x, from the column
    u = __fsub_rn(__fmul_rn(two_over_h, (float)i), 1.f);       // y, from the row
}

__global__ __launch_bounds__(THREADS) void boot_scale_fwd_kernel(
    const float *__restrict__ x, float *__restrict__ y, const float *__restrict__ rate,
    const float *__restrict__ center, int B, int C, int H, int W, float two_over_h, float two_over_w) {
    const size_t plane = (size_t)H * W;
    const size_t idx = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= (size_t)B * plane) return;
    const int b = (int)(idx / plane);
    const int p = (int)(idx - (size_t)b * plane);
    const int i = p / W, j = p - i * W;
    float v, u;
    base_grid(i, j, two_over_h, two_over_w, v, u);
    const float inv_rate = __fdiv_rn(1.f, rate[b]), cx = center[2 * b], cy = center[2 * b + 1];
    const float gx = __fadd_rn(__fmul_rn(inv_rate, __fsub_rn(v, cx)), cx);
    const float gy = __fadd_rn(__fmul_rn(inv_rate, __fsub_rn(u, cy)), cy);
    ScaleTaps tp;
    bicubic_taps(gx, gy, H, W, tp);
    for (int c = 0; c < C; ++c)
        y[((size_t)b * C + c) * plane + p] = bicubic_gather(x + (size_t)c * plane, W, tp);
}

// test.py's quantize_and_clamp in float32: a correctly rounded division, ties to even
__device__ __forceinline__ float quantize_clamp(float t) {
    const float q = __fdiv_rn(rintf(__fmul_rn(t, 255.f)), 255.f);
    return fminf(fmaxf(q, 0.f), 1.f);
}

__global__ __launch_bounds__(THREADS) void boot_luma_diff_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                                 size_t npix, int parts, float *__restrict__ d,
                                                                 float *__restrict__ work) {
    __shared__ float scratch[THREADS / 64];
    const size_t img = blockIdx.y;
    const float *pa = a + img * 3 * npix, *pb = b + img * 3 * npix;
    float *pd = d + img * npix;
    float s = 0.f;
    const size_t stride = (size_t)parts * THREADS;
    for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < npix; i += stride) {
        // luma_sqerr_kernel's expression (the file is built with -ffp-contract=off: unfused, left to right)
        const float ya = 0.299f * quantize_clamp(pa[i]) + 0.587f * quantize_clamp(pa[npix + i])
                         + 0.114f * quantize_clamp(pa[2 * npix + i]);
        const float yb = 0.299f * quantize_clamp(pb[i]) + 0.587f * quantize_clamp(pb[npix + i])
                         + 0.114f * quantize_clamp(pb[2 * npix + i]);
        const float e = ya - yb;
        pd[i] = e;
        s = fmaf(e, e, s);
    }
    const float bs = sei_block_sum<THREADS>(s, scratch);
    if (threadIdx.x == 0) work[img * parts + blockIdx.x] = bs;
}

// one workgroup of one wave per image: its partial sums in index order per lane, then the lanes, in double
__global__ __launch_bounds__(64) void boot_luma_sum_kernel(const float *__restrict__ work, int parts,
                                                           float *__restrict__ out) {
    const float *w = work + (size_t)blockIdx.x * parts;
    double s = 0.0;
    for (int i = threadIdx.x; i < parts; i += 64) s += (double)w[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (threadIdx.x == 0) out[blockIdx.x] = (float)s;
}

__global__ __launch_bounds__(THREADS) void boot_pullback_accum_kernel(
    const float *__restrict__ d, const float *__restrict__ rate, const float *__restrict__ center, int B, int H, int W,
    float two_over_h, float two_over_w, float *__restrict__ msq, int accumulate) {
    const size_t plane = (size_t)H * W;
    const size_t idx = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= plane) return;
    const int p = (int)idx;
    const int i = p / W, j = p - i * W;
    float v, u;
    base_grid(i, j, two_over_h, two_over_w, v, u);
    float acc = accumulate ? msq[p] : 0.f;
    for (int r = 0; r < B; ++r) {
        const float rho = rate[r], cx = center[2 * r], cy = center[2 * r + 1];
        const float gx = __fadd_rn(__fmul_rn(rho, __fsub_rn(v, cx)), cx);
        const float gy = __fadd_rn(__fmul_rn(rho, __fsub_rn(u, cy)), cy);
        ScaleTaps tp;
        bicubic_taps(gx, gy, H, W, tp);
        const float e = bicubic_gather(d + (size_t)r * plane, W, tp);
        acc = fmaf(e, e, acc);
    }
    msq[p] = acc;
}

// partial sums of one image: a function of its pixel count alone
int luma_parts(size_t npix) { return (int)sei_capped_grid(npix, THREADS, MAX_PARTS); }

bool extents_ok(int B, int H, int W) {
    // a pixel index is an int, and the grid of B planes stays below 2^31 workgroups
    return B > 0 && H > 0 && W > 0 && (size_t)H * W < ((size_t)1 << 30) &&
           sei_ceil_div((size_t)B * H * W, THREADS) < ((size_t)1 << 31);
}

}  // namespace

extern "C" int sei_boot_scale_fwd(const float *x, float *y, const float *rate, const float *center, int B, int C, int H,
                                  int W, void *stream) {
    SEI_REQUIRE(x && y && rate && center && x != y);
    SEI_REQUIRE(C > 0 && extents_ok(B, H, W));
    // python: 2 / w evaluated in double, then rounded to float32 when it multiplies a float tensor
    const float two_over_h = (float)(2.0 / (double)H), two_over_w = (float)(2.0 / (double)W);
    const size_t total = (size_t)B * H * W;
    hipLaunchKernelGGL(boot_scale_fwd_kernel, dim3((unsigned)sei_ceil_div(total, THREADS)), dim3(THREADS), 0,
                       (hipStream_t)stream, x, y, rate, center, B, C, H, W, two_over_h, two_over_w);
    return sei_launch_status();
}

extern "C" size_t sei_boot_luma_diff_work_floats(int batch, size_t npix) {
    if (batch < 1 || batch > 65535 || npix < 1 || npix >= ((size_t)1 << 30)) return 0;
    return (size_t)batch * luma_parts(npix);
}

extern "C" int sei_boot_luma_diff(const float *a, const float *b, int batch, size_t npix, float *d, float *out,
                                  float *work, void *stream) {
    SEI_REQUIRE(a && b && d && out && work);
    SEI_REQUIRE(sei_boot_luma_diff_work_floats(batch, npix) > 0);
    const int parts = luma_parts(npix);
    hipLaunchKernelGGL(boot_luma_diff_kernel, dim3(parts, batch), dim3(THREADS), 0, (hipStream_t)stream, a, b, npix, parts,
                       d, work);
    hipLaunchKernelGGL(boot_luma_sum_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, (const float *)work, parts,
                       out);
    return sei_launch_status();
}

extern "C" int sei_boot_pullback_accum(const float *d, const float *rate, const float *center, int B, int H, int W,
                                       float *msq, int accumulate, void *stream) {
    SEI_REQUIRE(d && rate && center && msq && d != msq);
    SEI_REQUIRE(extents_ok(B, H, W));
    const float two_over_h = (float)(2.0 / (double)H), two_over_w = (float)(2.0 / (double)W);
    hipLaunchKernelGGL(boot_pullback_accum_kernel, dim3((unsigned)sei_ceil_div((size_t)H * W, THREADS)), dim3(THREADS), 0,
                       (hipStream_t)stream, d, rate, center, B, H, W, two_over_h, two_over_w, msq, accumulate);
    return sei_launch_status();
}
