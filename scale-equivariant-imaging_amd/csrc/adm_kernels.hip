// The guided-diffusion ("ADM") U-Net of the DiffPIR_DiffUNet baseline (models/diffunet.py) for gfx950: GroupNorm + SiLU
// residual blocks with timestep scale-shift, biased 3x3 convolutions at 128 .. 1024 input channels, blocks that resample
// inside, and global self-attention with 64-wide heads.
//
// Layout: that of csrc/grid_conv.h. The trunk and every convolution result are float32 channels-last on the row
// indexing of a zero-bordered grid (B, H + 2, W + 2, C), R = B (H + 2) (W + 2) rows; the input of a convolution is a bf16
// grid of the same rows with W + 3 guard rows in front and behind; weights are bf16, tap-major (N, taps * Cin),
// K-contiguous. Every kernel reads and writes INTERIOR rows only (the packed image grid excepted, which is written whole):
// the border of a bf16 grid stays as the caller zeroed it, the border rows of a float32 buffer are never read.
//
//   adm_gn_stats_kernel   mean and 1 / sqrt(var + eps) per (image, group): two passes (a mean, then the distances from it)
//                         per slice of 1024 pixels, one workgroup each, and a fixed-order merge of the slices: no atomics,
//                         no E[x^2] - E[x]^2, a grid that depends on the extents only. The input may be the
//                         channel concatenation of two trunks (the U-Net skip), a group may straddle the seam.
//   adm_gn_apply_kernel   [SiLU](((x - mean) rstd gamma + beta) [* (1 + scale) + shift]) of that (concatenated) input, written
//                         as the bf16 grid of the next convolution and / or as float32, at the same extents, 2x2-averaged
//                         into the half extents or repeated 2x into the double ones; without statistics it is the plain
//                         copy / resampling of the residual path R(x) (and the bf16 copy the 1x1 skip convolution reads).
//   adm_conv_kernel       the implicit GEMM of grid_conv.h with any Cin that is a multiple of 32 (384 and 768 have 12 and 24
//                         steps per tap, no power of two), 9 taps or 1, and the epilogue (acc + bias) [+ residual] -> float32
//                         and / or bf16; the tail writes 3 channels of an NCHW image.
//   adm_attention_kernel  softmax((q^T k) / 8) v per head over all T = H W tokens of an image, flash style: one wave per 16
//                         queries walks the keys in tiles of 32, scores and the output on bf16 MFMA, the running row maximum
//                         and sum in float32, the probabilities rounded to bf16 for the second product.
#include "grid_conv.h"

#include <math.h>

namespace {

constexpr int ADM_GROUPS = 32;

bool adm_channels(int Ca, int Cb) {          // the concatenation has whole groups of a multiple of 4 channels
    return Ca >= 4 && Cb >= 0 && Ca % 4 == 0 && Cb % 4 == 0 && (Ca + Cb) % (4 * ADM_GROUPS) == 0 && Ca + Cb <= 4096;
}

struct AdmSrc {
    const float *Xa, *Xb;                    // (R, Ca) and (R, Cb) or NULL: channel c of the input is Xa's below Ca
    int Ca, Cb;
};
__device__ __forceinline__ f32x4 adm_read4(const AdmSrc &s, long long row, int c) {
    const float *p = c < s.Ca ? s.Xa + row * s.Ca + c : s.Xb + row * s.Cb + (c - s.Ca);
    return *reinterpret_cast<const f32x4 *>(p);
}
__device__ __forceinline__ long long adm_grid_row(int b, int i, int j, int H, int W) {     // interior pixel (i, j)
    return ((long long)b * (H + 2) + i + 1) * (W + 2) + j + 1;
}

// ---- GroupNorm statistics ----
// A group is cut into slices of ADM_GN_SLICE pixels, one workgroup per (group, image, slice): the workgroup's own two-pass
// mean and sum of squared distances. One slice (up to 1024 pixels): the statistics are written at once. More: the slices'
// (mean, M2) go to `part` and adm_gn_merge_kernel joins them in a fixed order (Chan's formula with every term
// non-negative). The grid depends on the extents only.
constexpr int ADM_GN_THREADS = 256, ADM_GN_SLICE = 1024;
int adm_gn_slices(int H, int W) { return (int)sei_ceil_div((size_t)H * W, ADM_GN_SLICE); }

__global__ __launch_bounds__(ADM_GN_THREADS) void adm_gn_stats_kernel(const AdmSrc src, int H, int W, float eps, float *stats,
                                                                      float *part) {
    __shared__ float scratch[ADM_GN_THREADS / 64];
    __shared__ float bcast;
    const int g = blockIdx.x, b = blockIdx.y, slices = gridDim.z;
    const int cg = (src.Ca + src.Cb) / ADM_GROUPS, q = cg / 4;       // channels of a group, float4 pieces of a pixel's group
    const int p0 = blockIdx.z * ADM_GN_SLICE, pixels = min(H * W - p0, ADM_GN_SLICE);
    const int items = pixels * q;
    float sum = 0.f;
    for (int i = threadIdx.x; i < items; i += ADM_GN_THREADS) {
        const int piece = i % q, p = p0 + i / q;
        const f32x4 v = adm_read4(src, adm_grid_row(b, p / W, p % W, H, W), g * cg + 4 * piece);
        sum += (v[0] + v[1]) + (v[2] + v[3]);
    }
    sum = sei_block_sum<ADM_GN_THREADS>(sum, scratch);
    if (threadIdx.x == 0) bcast = sum / (float)(items * 4);
    __syncthreads();
    // The second pass sums the distances d from that first mean m0 and their squares: the mean is m0 + E[d] (the first
    // pass's rounding, which grows with |m0| and the slice's size, corrected) and the sum of squared distances from it
    // sum(d^2) - n E[d]^2, where E[d] is a rounding error, so nothing cancels.
    const float m0 = bcast;
    float sd = 0.f, sq = 0.f;
    for (int i = threadIdx.x; i < items; i += ADM_GN_THREADS) {
        const int piece = i % q, p = p0 + i / q;
        const f32x4 v = adm_read4(src, adm_grid_row(b, p / W, p % W, H, W), g * cg + 4 * piece);
        const float d0 = v[0] - m0, d1 = v[1] - m0, d2 = v[2] - m0, d3 = v[3] - m0;
        sd += (d0 + d1) + (d2 + d3);
        sq += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
    sd = sei_block_sum<ADM_GN_THREADS>(sd, scratch);
    sq = sei_block_sum<ADM_GN_THREADS>(sq, scratch);
    if (threadIdx.x == 0) {
        const float n = (float)(items * 4), delta = sd / n;
        const float mean = m0 + delta, m2 = sq - n * (delta * delta);
        if (slices == 1) {
            stats[2 * (b * ADM_GROUPS + g)] = mean;
            stats[2 * (b * ADM_GROUPS + g) + 1] = 1.0f / sqrtf(m2 / n + eps);
        } else {
            float *o = part + 2 * ((size_t)(b * ADM_GROUPS + g) * slices + blockIdx.z);
            o[0] = mean;
            o[1] = m2;
        }
    }
}

// One wave per (group, image): mean = m_ref + sum n_s (mean_s - m_ref) / n with m_ref the first slice's mean (the differences
// are small, so the sum is exact to their size), then M2 = sum (M2_s + n_s (mean_s - mean)^2).
__global__ __launch_bounds__(64) void adm_gn_merge_kernel(const float *part, int slices, int H, int W, int cg, float eps,
                                                          float *stats) {
    const int g = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const float *p = part + 2 * (size_t)(b * ADM_GROUPS + g) * slices;
    const float mref = p[0], n = (float)H * (float)W * (float)cg;
    auto count = [&](int s) { return (float)(min(H * W - s * ADM_GN_SLICE, ADM_GN_SLICE) * cg); };
    float acc = 0.f;
    for (int s = lane; s < slices; s += 64) acc += count(s) * (p[2 * s] - mref);
    acc = sei_group_sum<64>(acc);
    const float mean = mref + acc / n;
    float m2 = 0.f;
    for (int s = lane; s < slices; s += 64) {
        const float d = p[2 * s] - mean;
        m2 += p[2 * s + 1] + count(s) * (d * d);
    }
    m2 = sei_group_sum<64>(m2);
    if (lane == 0) {
        stats[2 * (b * ADM_GROUPS + g)] = mean;
        stats[2 * (b * ADM_GROUPS + g) + 1] = 1.0f / sqrtf(m2 / n + eps);
    }
}

// ---- GroupNorm apply / resampling ----
enum { ADM_SAME = 0, ADM_DOWN = 1, ADM_UP = 2 };
struct AdmApply {
    AdmSrc src;
    const float *stats, *gamma, *beta, *mod;  // stats NULL: the plain copy; mod (B, 2 C): scale | shift, or NULL
    uint16_t *Y16;                            // row 0 of the output's bf16 grid, or NULL
    float *Y32;                               // the output's float32 rows, or NULL
    int B, H, W, resample, silu;              // H, W: the INPUT's extents; silu 0: the normalisation alone
};
__device__ __forceinline__ float adm_silu(float v) { return v / (1.0f + expf(-v)); }

__global__ __launch_bounds__(256) void adm_gn_apply_kernel(const AdmApply a) {
    const int C = a.src.Ca + a.src.Cb, q = C / 4, cg = C / ADM_GROUPS;
    const int Ho = a.resample == ADM_DOWN ? a.H / 2 : a.resample == ADM_UP ? 2 * a.H : a.H;
    const int Wo = a.resample == ADM_DOWN ? a.W / 2 : a.resample == ADM_UP ? 2 * a.W : a.W;
    const long long items = (long long)a.B * Ho * Wo * q;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (long long)gridDim.x * blockDim.x) {
        const int c = 4 * (int)(i % q);
        const long long p = i / q;
        const int jo = (int)(p % Wo), io = (int)((p / Wo) % Ho), b = (int)(p / ((long long)Wo * Ho));
        f32x4 ga{1.f, 1.f, 1.f, 1.f}, be{0.f, 0.f, 0.f, 0.f}, sc{0.f, 0.f, 0.f, 0.f}, sh{0.f, 0.f, 0.f, 0.f};
        float mean = 0.f, rstd = 1.f;
        if (a.stats) {
            const int g = c / cg;                                     // (cg is a multiple of 4: the four share a group)
            mean = a.stats[2 * (b * ADM_GROUPS + g)];
            rstd = a.stats[2 * (b * ADM_GROUPS + g) + 1];
            ga = *reinterpret_cast<const f32x4 *>(a.gamma + c);
            be = *reinterpret_cast<const f32x4 *>(a.beta + c);
            if (a.mod) {
                sc = *reinterpret_cast<const f32x4 *>(a.mod + (size_t)b * 2 * C + c);
                sh = *reinterpret_cast<const f32x4 *>(a.mod + (size_t)b * 2 * C + C + c);
            }
        }
        auto value = [&](int ii, int jj) {
            f32x4 v = adm_read4(a.src, adm_grid_row(b, ii, jj, a.H, a.W), c);
            if (a.stats) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = (v[e] - mean) * rstd * ga[e] + be[e];
                    if (a.mod) t = t * (1.0f + sc[e]) + sh[e];
                    v[e] = a.silu ? adm_silu(t) : t;
                }
            }
            return v;
        };
        f32x4 r;
        if (a.resample == ADM_DOWN) {
            const f32x4 v00 = value(2 * io, 2 * jo), v01 = value(2 * io, 2 * jo + 1);
            const f32x4 v10 = value(2 * io + 1, 2 * jo), v11 = value(2 * io + 1, 2 * jo + 1);
            r = ((v00 + v01) + (v10 + v11)) * 0.25f;
        } else if (a.resample == ADM_UP) {
            r = value(io >> 1, jo >> 1);
        } else {
            r = value(io, jo);
        }
        const size_t at = (size_t)adm_grid_row(b, io, jo, Ho, Wo) * C + c;
        if (a.Y32) *reinterpret_cast<f32x4 *>(a.Y32 + at) = r;
        if (a.Y16) *reinterpret_cast<u32x2 *>(a.Y16 + at) = u32x2{sei_pack2_bf16(r[0], r[1]), sei_pack2_bf16(r[2], r[3])};
    }
}

// ---- the convolution ----
enum { ADM_EPI_TRUNK = 0, ADM_EPI_TAIL = 1 };
struct AdmConv {
    const uint16_t *X;                       // row 0 of the input grid
    const uint16_t *Wt;                      // (N, ntaps * Cin)
    const float *bias;                       // N entries
    const float *Tres;                       // optional addend on the output's rows
    float *Tout;                             // float32 rows, or NULL; the tail: the NCHW image
    uint16_t *Y16;                           // bf16 rows, or NULL
    int Cin, ntaps, N, M;                    // M = rows of the grid
    int H, W;
    int Cout;                                // the tail: channels of the image
};

// grid_conv with any count of steps per tap (Cin / 32) and the family's epilogue
template <int NB, int PB, int EPI>
__global__ __launch_bounds__(64) void adm_conv_kernel(const AdmConv a) {
    const GridConv core{a.X, a.Wt, a.Cin, a.ntaps, a.N, a.M, a.H, a.W};
    grid_conv<NB, PB, false, false>(core, [&](const GridRow &r, int n, f32x4 acc) {
        f32x4 v = acc + *reinterpret_cast<const f32x4 *>(a.bias + n);
        if (EPI == ADM_EPI_TRUNK) {
            const size_t at = (size_t)r.row * a.N + n;
            if (a.Tres) v = v + *reinterpret_cast<const f32x4 *>(a.Tres + at);
            if (a.Tout) *reinterpret_cast<f32x4 *>(a.Tout + at) = v;
            if (a.Y16) *reinterpret_cast<u32x2 *>(a.Y16 + at) = u32x2{sei_pack2_bf16(v[0], v[1]), sei_pack2_bf16(v[2], v[3])};
        } else {
            grid_store_nchw(a.Tout, a.Cout, a.H, a.W, r, n, v);
        }
    });
}

template <int NB, int EPI>
int adm_conv_launch(const AdmConv &a, hipStream_t s) {
    if (grid_default_pb(a.M, a.N, NB) == 4)
        hipLaunchKernelGGL((adm_conv_kernel<NB, 4, EPI>), (grid_conv_waves<NB, 4>(a.M, a.N)), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((adm_conv_kernel<NB, 2, EPI>), (grid_conv_waves<NB, 2>(a.M, a.N)), dim3(64), 0, s, a);
    return sei_launch_status();
}

// ---- attention ----
constexpr int ADM_HEAD_DIM = 64, ADM_KEYS = 32, ADM_VLD = 72;         // keys per tile; LDS row stride of the V tile (bf16)
__global__ __launch_bounds__(64) void adm_attention_kernel(const uint16_t *QKV, uint16_t *A16, int C, int H, int W) {
    __shared__ __attribute__((aligned(16))) uint16_t Vs[ADM_KEYS * ADM_VLD];
    const int lane = threadIdx.x, l16 = lane & 15, lg = lane >> 4;
    const int q0 = blockIdx.x * 16, head = blockIdx.y, b = blockIdx.z;
    const int T = H * W, ld = 3 * C;
    auto token_row = [&](int t) { return adm_grid_row(b, t / W, t % W, H, W); };
    const uint16_t *base = QKV + 3 * ADM_HEAD_DIM * head;            // q | k | v of this head, 64 channels each

    const int qt = min(q0 + l16, T - 1);
    const uint16_t *qp = base + token_row(qt) * ld + 8 * lg;
    const bf16x8 fq0 = *reinterpret_cast<const bf16x8 *>(qp), fq1 = *reinterpret_cast<const bf16x8 *>(qp + 32);

    f32x4 o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float mrun = -INFINITY, lrun = 0.f;                              // lrun: this lane's share of the row sum

    for (int k0 = 0; k0 < T; k0 += ADM_KEYS) {
        __syncthreads();                                             // the last tile's V has been read
#pragma unroll
        for (int r = 0; r < 4; ++r) {                                // the V tile: 32 keys x 64 channels, 16 bytes a piece
            const int idx = lane + 64 * r, key = idx >> 3, chunk = idx & 7;
            const uint16_t *vp = base + token_row(min(k0 + key, T - 1)) * ld + 2 * ADM_HEAD_DIM + 8 * chunk;
            *reinterpret_cast<u32x4 *>(Vs + key * ADM_VLD + 8 * chunk) = *reinterpret_cast<const u32x4 *>(vp);
        }
        f32x4 s[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {                             // S^T: keys k0 + 16 kt + 4 lg + e, query q0 + l16
            const uint16_t *kp = base + token_row(min(k0 + 16 * kt + l16, T - 1)) * ld + ADM_HEAD_DIM + 8 * lg;
            const bf16x8 fk0 = *reinterpret_cast<const bf16x8 *>(kp), fk1 = *reinterpret_cast<const bf16x8 *>(kp + 32);
            s[kt] = sei_mfma16(fk0, fq0, f32x4{0.f, 0.f, 0.f, 0.f});
            s[kt] = sei_mfma16(fk1, fq1, s[kt]);
        }
        float tmax = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s[kt][e] = k0 + 16 * kt + 4 * lg + e < T ? s[kt][e] * 0.125f : -INFINITY;
                tmax = fmaxf(tmax, s[kt][e]);
            }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));                // (a tile holds a valid key: tmax is finite)
        const float mnew = fmaxf(mrun, tmax), alpha = expf(mrun - mnew);
        mrun = mnew;
        float p[8], psum = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            p[i] = expf(s[i >> 2][i & 3] - mnew);
            psum += p[i];
        }
        lrun = lrun * alpha + psum;
        bf16x8 fp;                                                   // reduction slot i of lane group lg: key k0 + 16 (i / 4) + 4 lg + i % 4
#pragma unroll
        for (int i = 0; i < 8; ++i) fp[i] = (__bf16)p[i];
        __syncthreads();                                             // the V tile is in LDS
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v8s fv;
#pragma unroll
            for (int i = 0; i < 8; ++i) fv[i] = (short)Vs[(16 * (i >> 2) + 4 * lg + (i & 3)) * ADM_VLD + 16 * j + l16];
            o[j] = sei_mfma16(__builtin_bit_cast(bf16x8, fv), fp, o[j] * alpha);     // channel 16 j + 4 lg + e, query l16
        }
    }
    float lsum = lrun + __shfl_xor(lrun, 16, 64);
    lsum = lsum + __shfl_xor(lsum, 32, 64);
    if (q0 + l16 < T) {
        uint16_t *op = A16 + token_row(q0 + l16) * C + ADM_HEAD_DIM * head + 4 * lg;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 v = o[j] / lsum;
            *reinterpret_cast<u32x2 *>(op + 16 * j) = u32x2{sei_pack2_bf16(v[0], v[1]), sei_pack2_bf16(v[2], v[3])};
        }
    }
}

}  // namespace

extern "C" size_t sei_adm_gn_part_floats(int H, int W) {
    return grid_rows(1, H, W) ? (size_t)2 * ADM_GROUPS * adm_gn_slices(H, W) : 0;
}

extern "C" int sei_adm_gn_stats(const float *Xa, int Ca, const float *Xb, int Cb, int B, int H, int W, float eps, float *stats,
                                float *part, void *stream) {
    SEI_REQUIRE(Xa && stats && part && grid_al16(Xa) && grid_al16(Xb) && ((uintptr_t)stats & 3) == 0 && ((uintptr_t)part & 3) == 0);
    SEI_REQUIRE(adm_channels(Ca, Cb) && (Cb == 0) == (Xb == nullptr) && eps > 0.f);
    SEI_REQUIRE(grid_rows(B, H, W) > 0 && B <= 65535);
    const int slices = adm_gn_slices(H, W);
    SEI_REQUIRE(slices <= 65535);
    hipLaunchKernelGGL(adm_gn_stats_kernel, dim3(ADM_GROUPS, B, slices), dim3(ADM_GN_THREADS), 0, (hipStream_t)stream,
                       AdmSrc{Xa, Xb, Ca, Cb}, H, W, eps, stats, part);
    if (slices > 1)
        hipLaunchKernelGGL(adm_gn_merge_kernel, dim3(ADM_GROUPS, B), dim3(64), 0, (hipStream_t)stream, part, slices, H, W,
                           (Ca + Cb) / ADM_GROUPS, eps, stats);
    return sei_launch_status();
}

extern "C" int sei_adm_gn_apply(const float *Xa, int Ca, const float *Xb, int Cb, const float *stats, const float *gamma,
                                const float *beta, const float *mod, int silu, int B, int H, int W, int resample,
                                uint16_t *Y16, float *Y32, void *stream) {
    SEI_REQUIRE(Xa && (Y16 || Y32) && grid_al16(Xa) && grid_al16(Xb) && grid_al16(Y16) && grid_al16(Y32));
    SEI_REQUIRE(adm_channels(Ca, Cb) && (Cb == 0) == (Xb == nullptr));
    SEI_REQUIRE(Y32 != Xa && (!Xb || Y32 != Xb));
    if (stats) SEI_REQUIRE(gamma && beta && grid_al16(gamma) && grid_al16(beta) && grid_al16(mod) && ((uintptr_t)stats & 3) == 0);
    else SEI_REQUIRE(!gamma && !beta && !mod);
    SEI_REQUIRE((resample == ADM_SAME || resample == ADM_DOWN || resample == ADM_UP) && (silu == 0 || silu == 1));
    SEI_REQUIRE(grid_rows(B, H, W) > 0);
    if (resample == ADM_DOWN) SEI_REQUIRE(H % 2 == 0 && W % 2 == 0);
    if (resample == ADM_UP) SEI_REQUIRE(grid_rows(B, 2 * H, 2 * W) > 0);
    const int Ho = resample == ADM_DOWN ? H / 2 : resample == ADM_UP ? 2 * H : H;
    const int Wo = resample == ADM_DOWN ? W / 2 : resample == ADM_UP ? 2 * W : W;
    const size_t items = (size_t)B * Ho * Wo * ((Ca + Cb) / 4);
    AdmApply a{AdmSrc{Xa, Xb, Ca, Cb}, stats, gamma, beta, mod, Y16, Y32, B, H, W, resample, silu};
    hipLaunchKernelGGL(adm_gn_apply_kernel, dim3(sei_capped_grid(items, 256, 8192)), dim3(256), 0, (hipStream_t)stream, a);
    return sei_launch_status();
}

extern "C" int sei_adm_pack_image(const float *x, uint16_t *G16, int B, int H, int W, void *stream) {
    SEI_REQUIRE(x && G16 && ((uintptr_t)x & 3) == 0 && grid_al16(G16));
    const long long R = grid_rows(B, H, W);
    SEI_REQUIRE(R > 0);
    grid_pack_image(x, 0.f, G16, R, B, H, W, (hipStream_t)stream);          // channel 3: zero like the rest
    return sei_launch_status();
}

extern "C" int sei_adm_conv(const uint16_t *X, const uint16_t *Wt, const float *bias, int Cin, int Cout, int ntaps, int B, int H,
                            int W, const float *T_res, float *T_out, uint16_t *Y16, void *stream) {
    SEI_REQUIRE(X && Wt && bias && (T_out || Y16) && X != Y16 && grid_al16(X) && grid_al16(Wt) && grid_al16(bias) &&
                grid_al16(T_res) && grid_al16(T_out) && grid_al16(Y16));
    SEI_REQUIRE(Cin >= 32 && Cin % 32 == 0 && Cin <= 4096 && Cout >= 64 && Cout % 64 == 0 && Cout <= 8192);
    SEI_REQUIRE(ntaps == 1 || ntaps == 9);
    const long long R = grid_rows(B, H, W);
    SEI_REQUIRE(R > 0);
    AdmConv a{X, Wt, bias, T_res, T_out, Y16, Cin, ntaps, Cout, (int)R, H, W, Cout};
    return adm_conv_launch<4, ADM_EPI_TRUNK>(a, (hipStream_t)stream);
}

extern "C" int sei_adm_tail(const uint16_t *X, const uint16_t *Wt, const float *bias, int Cin, int B, int H, int W, float *out,
                            void *stream) {
    SEI_REQUIRE(X && Wt && bias && out && grid_al16(X) && grid_al16(Wt) && grid_al16(bias) && ((uintptr_t)out & 3) == 0);
    SEI_REQUIRE(Cin >= 32 && Cin % 32 == 0 && Cin <= 4096);
    const long long R = grid_rows(B, H, W);
    SEI_REQUIRE(R > 0);
    AdmConv a{X, Wt, bias, nullptr, out, nullptr, Cin, 9, 16, (int)R, H, W, 3};
    return adm_conv_launch<1, ADM_EPI_TAIL>(a, (hipStream_t)stream);
}

extern "C" int sei_adm_attention(const uint16_t *QKV16, int C, int B, int H, int W, uint16_t *A16, void *stream) {
    SEI_REQUIRE(QKV16 && A16 && grid_al16(QKV16) && grid_al16(A16));
    SEI_REQUIRE(C >= ADM_HEAD_DIM && C % ADM_HEAD_DIM == 0 && C <= 4096);
    SEI_REQUIRE(grid_rows(B, H, W) > 0 && B <= 65535 && (long long)H * W <= (1 << 20));
    const dim3 grid((unsigned)sei_ceil_div((size_t)H * W, 16), (unsigned)(C / ADM_HEAD_DIM), (unsigned)B);
    hipLaunchKernelGGL(adm_attention_kernel, grid, dim3(64), 0, (hipStream_t)stream, QKV16, A16, C, H, W);
    return sei_launch_status();
}
