// The DRUNet denoiser of the PlugAndPlay baseline (models/drunet.py) for gfx950: a bias-free ResNet-UNet of 3x3
// convolutions at 64 / 128 / 256 / 512 channels, 2x2 stride-2 convolutions down and 2x2 transposed convolutions up.
//
// Layout. Activations between convolutions are bf16 channels-last on zero-bordered grids (B, H + 2, W + 2, C) of
// R = B (H + 2) (W + 2) rows with W + 3 guard rows in front and behind (the layout of sei_pad_nhwc_bf16); the residual
// trunk T is float32 on the same row indexing. Weights are bf16, tap-major (N, taps * Cin), K-contiguous.
//
// One kernel body serves the whole family: an implicit GEMM D[n][r] = sum over taps t and channels c of
// Wt[n][t Cin + c] X[src_t(r)][c], the weights as the MFMA's A operand and the grid rows as its B operand, so a lane's
// four accumulator elements are four neighbouring CHANNELS of one grid row (16-byte float32 / 8-byte bf16 stores). Both
// operands are K-contiguous, so a lane's fragment (8 bf16 of one row) is ONE 16-byte global load: no LDS image, no
// barrier; the loads of two reduction steps ahead are in flight behind a step's MFMAs. (The LDS-DMA staged form of
// gemm_bf16nt.hip is the known next step; DESIGN 4.11 has the measured rates.)
// Every output element is one wave's k-ordered MFMA chain over its own row's inputs: no split-K, no atomics, the same
// bits on every run and wherever the image sits in the batch. Only interior rows are written: the border of an output
// grid stays as the caller zeroed it, guard rows are read (into results that are dropped) and never written.
//
// The network's vector-Jacobian product (models/drunet.py, for the DPS baseline) is the same family with transposed weights
// and one more epilogue, DR_MASK16: Y16 = bf16(conv(X)) where a taped bf16 grid (a ResBlock's ReLU output) is above zero,
// else 0 -- the first half of the block's backward (sei_drunet_conv3x3_masked).
#include "sei_common.h"

namespace {

enum { DR_SHIFT = 0, DR_DOWN = 1 };          // where tap t of row r reads: r + its row shift / the 2x2 gather
enum { DR_RELU16 = 0, DR_RES = 1, DR_UP = 2, DR_TAIL = 3, DR_MASK16 = 4 };

struct DrArgs {
    const uint16_t *X;                       // row 0 of the input grid
    const uint16_t *Wt;                      // (N, ntaps * Cin)
    const float *Tin, *Tskip;                // DR_RES: optional addends on the output grid's rows
    float *Tout;                             // DR_RES / DR_UP: trunk; DR_TAIL: the NCHW image
    uint16_t *Y16;                           // row 0 of the output grid
    int Cin, ntaps, N, M;                    // M = rows of the grid the launch walks
    int H, W;                                // interior extents of that grid
    int Cout;                                // DR_UP: N = 4 Cout; DR_TAIL: channels of the image
    const uint16_t *Mask;                    // DR_MASK16: row 0 of a bf16 grid of the output's shape, kept where it is > 0
};

// One wave per workgroup: PB 16-row blocks of grid rows x NB 16-channel blocks. The reduction runs in steps of 32 channels
// of one tap (Cin / 32 steps per tap, a power of two); a step's fragments are PB + NB 16-byte loads per lane, and the loads
// of the two steps ahead are in flight while a step's MFMAs run (three register sets): with one to six waves per SIMD
// there is little else to hide the L2 latency behind.
template <int NB, int PB, int GATHER, int EPI>
__global__ __launch_bounds__(64) void drunet_gemm_kernel(const DrArgs a) {
    const int lane = threadIdx.x, l16 = lane & 15, lg = lane >> 4;
    const int m0 = blockIdx.x * (16 * PB), n0 = blockIdx.y * (16 * NB);
    const int Hp = a.H + 2, Wp = a.W + 2;
    int mrow[PB], bi[PB], ii[PB], jj[PB];
    bool ok[PB];
    const uint16_t *xb[PB], *wb[NB];
#pragma unroll
    for (int p = 0; p < PB; ++p) {
        const int m = m0 + 16 * p + l16;
        mrow[p] = min(m, a.M - 1);           // rows past the end read the last row and store nothing
        jj[p] = mrow[p] % Wp;
        const int q = mrow[p] / Wp;
        ii[p] = q % Hp;
        bi[p] = q / Hp;
        ok[p] = m < a.M && ii[p] >= 1 && ii[p] <= a.H && jj[p] >= 1 && jj[p] <= a.W;
        long long src = mrow[p];             // DR_SHIFT: the row itself, every tap adds its shift
        if (GATHER == DR_DOWN)               // tap (0, 0) of the 2x2 patch; a border row reads (and drops) the patch at row 0
            src = ok[p] ? ((long long)bi[p] * (2 * a.H + 2) + 2 * ii[p] - 1) * (2 * a.W + 2) + 2 * jj[p] - 1 : 0;
        xb[p] = a.X + src * a.Cin + 8 * lg;
    }
    const size_t K = (size_t)a.ntaps * a.Cin;
#pragma unroll
    for (int j = 0; j < NB; ++j) wb[j] = a.Wt + (size_t)(n0 + 16 * j + l16) * K + 8 * lg;

    f32x4 acc[NB][PB];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int p = 0; p < PB; ++p) acc[j][p] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int spt = a.Cin >> 5, spt_log2 = 31 - __builtin_clz(spt), total = a.ntaps * spt;
    const int in_w = GATHER == DR_DOWN ? 2 * a.W + 2 : Wp;
    auto load = [&](int s, bf16x8(&fx)[PB], bf16x8(&fw)[NB]) {
        const int t = s >> spt_log2, c0 = (s & (spt - 1)) << 5;          // wave-uniform
        int shift;                                                       // grid rows from the base row to tap t
        if (GATHER == DR_DOWN) shift = (t >> 1) * in_w + (t & 1);
        else shift = a.ntaps == 1 ? 0 : (t / 3 - 1) * in_w + (t % 3 - 1);
        const long long off = (long long)shift * a.Cin + c0;
#pragma unroll
        for (int p = 0; p < PB; ++p) fx[p] = *reinterpret_cast<const bf16x8 *>(xb[p] + off);
#pragma unroll
        for (int j = 0; j < NB; ++j) fw[j] = *reinterpret_cast<const bf16x8 *>(wb[j] + (size_t)s * 32);
    };
    auto mma = [&](const bf16x8(&fx)[PB], const bf16x8(&fw)[NB]) {
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int p = 0; p < PB; ++p) acc[j][p] = sei_mfma16(fw[j], fx[p], acc[j][p]);
    };
    bf16x8 x0[PB], x1[PB], x2[PB], w0[NB], w1[NB], w2[NB];
    // (loads past the end repeat the last step instead of branching around it: with conditional loads the compiler
    // cannot count what is in flight and drains everything before the first MFMA of every turn)
    const int last = total - 1;
    load(0, x0, w0);
    load(min(1, last), x1, w1);
    for (int s = 0; s < total; s += 3) {
        load(min(s + 2, last), x2, w2);
        mma(x0, w0);
        if (s + 1 >= total) break;
        load(min(s + 3, last), x0, w0);
        mma(x1, w1);
        if (s + 2 >= total) break;
        load(min(s + 4, last), x1, w1);
        mma(x2, w2);
    }

    // accumulator element e of block (j, p): channel n0 + 16 j + 4 lg + e of grid row m0 + 16 p + l16
#pragma unroll
    for (int p = 0; p < PB; ++p) {
        if (!ok[p]) continue;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int n = n0 + 16 * j + 4 * lg;
            f32x4 v = acc[j][p];
            if (EPI == DR_RELU16) {
                const size_t at = (size_t)mrow[p] * a.N + n;
                *reinterpret_cast<u32x2 *>(a.Y16 + at) =
                    u32x2{sei_pack2_bf16(fmaxf(v[0], 0.f), fmaxf(v[1], 0.f)), sei_pack2_bf16(fmaxf(v[2], 0.f), fmaxf(v[3], 0.f))};
            } else if (EPI == DR_MASK16) {             // the ResBlock's backward: the ReLU's derivative from its taped output
                const size_t at = (size_t)mrow[p] * a.N + n;
                const u32x2 m = *reinterpret_cast<const u32x2 *>(a.Mask + at);
#pragma unroll
                for (int e = 0; e < 4; ++e)            // a bf16 is above zero when its bits, read as int16, are
                    if ((int16_t)(m[e >> 1] >> (16 * (e & 1))) <= 0) v[e] = 0.f;
                *reinterpret_cast<u32x2 *>(a.Y16 + at) = u32x2{sei_pack2_bf16(v[0], v[1]), sei_pack2_bf16(v[2], v[3])};
            } else if (EPI == DR_RES) {
                const size_t at = (size_t)mrow[p] * a.N + n;
                if (a.Tin) v = *reinterpret_cast<const f32x4 *>(a.Tin + at) + v;
                if (a.Tskip) v = v + *reinterpret_cast<const f32x4 *>(a.Tskip + at);
                *reinterpret_cast<f32x4 *>(a.Tout + at) = v;
                *reinterpret_cast<u32x2 *>(a.Y16 + at) = u32x2{sei_pack2_bf16(v[0], v[1]), sei_pack2_bf16(v[2], v[3])};
            } else if (EPI == DR_UP) {
                const int tap = n / a.Cout, co = n - tap * a.Cout;
                const long long dst = ((long long)bi[p] * (2 * a.H + 2) + 2 * ii[p] - 1 + (tap >> 1)) * (2 * a.W + 2) +
                                      2 * jj[p] - 1 + (tap & 1);
                const size_t at = (size_t)dst * a.Cout + co;
                *reinterpret_cast<f32x4 *>(a.Tout + at) = v;
                *reinterpret_cast<u32x2 *>(a.Y16 + at) = u32x2{sei_pack2_bf16(v[0], v[1]), sei_pack2_bf16(v[2], v[3])};
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (n + e < a.Cout)
                        a.Tout[(((size_t)bi[p] * a.Cout + n + e) * a.H + (ii[p] - 1)) * a.W + (jj[p] - 1)] = v[e];
            }
        }
    }
}

// x (B, 3, H, W) float32 and the noise level -> the head's input grid: 32 channels (x, sigma, zeros) per row, border rows
// zero. The constant channel is zero on the border like the image, which is why it is no bias.
constexpr int DR_HEAD_CIN = 32;
__global__ void drunet_head_pack_kernel(const float *x, float sigma, uint16_t *g, int B, int H, int W) {
    const int Hp = H + 2, Wp = W + 2;
    const size_t n = (size_t)B * Hp * Wp * (DR_HEAD_CIN / 8);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int chunk = (int)(i % (DR_HEAD_CIN / 8));
        const size_t r = i / (DR_HEAD_CIN / 8);
        const int j = (int)(r % Wp), q = (int)(r / Wp), ii = q % Hp, b = q / Hp;
        u32x4 v{0u, 0u, 0u, 0u};
        if (chunk == 0 && ii >= 1 && ii <= H && j >= 1 && j <= W) {
            const size_t plane = (size_t)H * W, at = (size_t)b * 3 * plane + (size_t)(ii - 1) * W + (j - 1);
            v[0] = sei_pack2_bf16(x[at], x[at + plane]);
            v[1] = sei_pack2_bf16(x[at + 2 * plane], sigma);
        }
        *reinterpret_cast<u32x4 *>(g + r * DR_HEAD_CIN + 8 * chunk) = v;
    }
}

bool dr_width(int c) { return c == 64 || c == 128 || c == 256 || c == 512; }
bool dr_al16(const void *p) { return ((uintptr_t)p & 15) == 0; }
// rows of the zero-bordered grid of B images of H x W, 0 when the arguments are refused (or the row count leaves int)
long long dr_rows(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1 || H > 16384 || W > 16384) return 0;
    const long long r = (long long)B * (H + 2) * (W + 2);
    return r < (1ll << 30) ? r : 0;
}

template <int NB, int PB, int GATHER, int EPI>
int dr_launch_pb(const DrArgs &a, hipStream_t s) {
    const dim3 grid((unsigned)sei_ceil_div((size_t)a.M, 16 * PB), (unsigned)(a.N / (16 * NB)));
    hipLaunchKernelGGL((drunet_gemm_kernel<NB, PB, GATHER, EPI>), grid, dim3(64), 0, s, a);
    return sei_launch_status();
}

// Grid rows per wave: 16 pb. The measured table (tools/exp_drunet.py): 64 rows win wherever they leave the
// launch 392 waves or more (levels 0 - 2 of a 256 x 384 image and of 32 patches of 48 x 48) and lose to 32 rows at 216 and
// 256 waves (level 3 of either: fewer waves than the chip has CUs); 16 rows never won. So: 64 rows when that gives
// DR_MIN_WAVES waves, else 32. pb = 1 stays reachable through sei_drunet_conv3x3_ex.
constexpr long long DR_MIN_WAVES = 320;
bool dr_pb_ok(int pb) { return pb == 1 || pb == 2 || pb == 4; }
int dr_default_pb(long long rows, int N, int nb) {
    return (long long)sei_ceil_div((size_t)rows, 64) * (N / (16 * nb)) >= DR_MIN_WAVES ? 4 : 2;
}
template <int NB, int GATHER, int EPI>
int dr_launch(const DrArgs &a, int pb, hipStream_t s) {
    if (pb == 0) pb = dr_default_pb(a.M, a.N, NB);
    switch (pb) {
        case 1: return dr_launch_pb<NB, 1, GATHER, EPI>(a, s);
        case 2: return dr_launch_pb<NB, 2, GATHER, EPI>(a, s);
        default: return dr_launch_pb<NB, 4, GATHER, EPI>(a, s);
    }
}

}  // namespace

extern "C" size_t sei_drunet_work_bytes(int B, int H, int W) {
    const long long r = dr_rows(B, H, W);
    return r ? (size_t)(r + 2 * (W + 3)) * DR_HEAD_CIN * sizeof(uint16_t) : 0;
}

extern "C" int sei_drunet_conv3x3_ex(const uint16_t *X, const uint16_t *Wt, int Cin, int Cout, int B, int H, int W,
                                     int epilogue, const float *T_in, const float *T_skip, float *T_out, uint16_t *Y16,
                                     int pb, void *stream) {
    SEI_REQUIRE(pb == 0 || dr_pb_ok(pb));
    SEI_REQUIRE(X && Wt && Y16 && X != Y16 && dr_al16(X) && dr_al16(Wt) && dr_al16(Y16));
    SEI_REQUIRE(dr_width(Cin) && dr_width(Cout) && (epilogue == 0 || epilogue == 1));
    const long long R = dr_rows(B, H, W);
    SEI_REQUIRE(R > 0);
    if (epilogue == 0) SEI_REQUIRE(!T_in && !T_skip && !T_out);
    else SEI_REQUIRE(T_in && T_out && dr_al16(T_in) && dr_al16(T_skip) && dr_al16(T_out));
    DrArgs a{X, Wt, T_in, T_skip, T_out, Y16, Cin, 9, Cout, (int)R, H, W, Cout};
    return epilogue == 0 ? dr_launch<4, DR_SHIFT, DR_RELU16>(a, pb, (hipStream_t)stream)
                         : dr_launch<4, DR_SHIFT, DR_RES>(a, pb, (hipStream_t)stream);
}

extern "C" int sei_drunet_conv3x3(const uint16_t *X, const uint16_t *Wt, int Cin, int Cout, int B, int H, int W, int epilogue,
                                  const float *T_in, const float *T_skip, float *T_out, uint16_t *Y16, void *stream) {
    return sei_drunet_conv3x3_ex(X, Wt, Cin, Cout, B, H, W, epilogue, T_in, T_skip, T_out, Y16, 0, stream);
}

extern "C" int sei_drunet_conv3x3_masked_ex(const uint16_t *X, const uint16_t *Wt, int Cin, int Cout, int B, int H, int W,
                                            const uint16_t *Mask, uint16_t *Y16, int pb, void *stream) {
    SEI_REQUIRE(pb == 0 || dr_pb_ok(pb));
    SEI_REQUIRE(X && Wt && Mask && Y16 && X != Y16 && Mask != Y16 && dr_al16(X) && dr_al16(Wt) && dr_al16(Mask) && dr_al16(Y16));
    SEI_REQUIRE(dr_width(Cin) && dr_width(Cout));
    const long long R = dr_rows(B, H, W);
    SEI_REQUIRE(R > 0);
    DrArgs a{X, Wt, nullptr, nullptr, nullptr, Y16, Cin, 9, Cout, (int)R, H, W, Cout, Mask};
    return dr_launch<4, DR_SHIFT, DR_MASK16>(a, pb, (hipStream_t)stream);
}

extern "C" int sei_drunet_conv3x3_masked(const uint16_t *X, const uint16_t *Wt, int Cin, int Cout, int B, int H, int W,
                                         const uint16_t *Mask, uint16_t *Y16, void *stream) {
    return sei_drunet_conv3x3_masked_ex(X, Wt, Cin, Cout, B, H, W, Mask, Y16, 0, stream);
}

extern "C" int sei_drunet_down(const uint16_t *X, const uint16_t *Wt, int Cin, int Cout, int B, int Ho, int Wo, float *T_out,
                               uint16_t *Y16, void *stream) {
    SEI_REQUIRE(X && Wt && T_out && Y16 && X != Y16 && dr_al16(X) && dr_al16(Wt) && dr_al16(T_out) && dr_al16(Y16));
    SEI_REQUIRE(dr_width(Cin) && dr_width(Cout));
    const long long R = dr_rows(B, Ho, Wo);
    SEI_REQUIRE(R > 0 && dr_rows(B, 2 * Ho, 2 * Wo) > 0);
    DrArgs a{X, Wt, nullptr, nullptr, T_out, Y16, Cin, 4, Cout, (int)R, Ho, Wo, Cout};
    return dr_launch<4, DR_DOWN, DR_RES>(a, 0, (hipStream_t)stream);
}

extern "C" int sei_drunet_up(const uint16_t *X, const uint16_t *Wt, int Cin, int Cout, int B, int H, int W, float *T_out,
                             uint16_t *Y16, void *stream) {
    SEI_REQUIRE(X && Wt && T_out && Y16 && X != Y16 && dr_al16(X) && dr_al16(Wt) && dr_al16(T_out) && dr_al16(Y16));
    SEI_REQUIRE(dr_width(Cin) && dr_width(Cout));
    const long long R = dr_rows(B, H, W);
    SEI_REQUIRE(R > 0 && dr_rows(B, 2 * H, 2 * W) > 0);
    DrArgs a{X, Wt, nullptr, nullptr, T_out, Y16, Cin, 1, 4 * Cout, (int)R, H, W, Cout};
    return dr_launch<4, DR_SHIFT, DR_UP>(a, 0, (hipStream_t)stream);
}

extern "C" int sei_drunet_head(const float *x, float sigma, const uint16_t *Wt, int Cout, int B, int H, int W, float *T_out,
                               uint16_t *Y16, void *work, void *stream) {
    SEI_REQUIRE(x && Wt && T_out && Y16 && work && ((uintptr_t)x & 3) == 0 && dr_al16(Wt) && dr_al16(T_out) &&
                dr_al16(Y16) && dr_al16(work));
    SEI_REQUIRE(dr_width(Cout) && sigma == sigma);
    const long long R = dr_rows(B, H, W);
    SEI_REQUIRE(R > 0);
    hipStream_t s = (hipStream_t)stream;
    uint16_t *grid = reinterpret_cast<uint16_t *>(work) + (size_t)(W + 3) * DR_HEAD_CIN;
    hipLaunchKernelGGL(drunet_head_pack_kernel, dim3(sei_capped_grid((size_t)R * (DR_HEAD_CIN / 8), 256, 4096)), dim3(256), 0,
                       s, x, sigma, grid, B, H, W);
    DrArgs a{grid, Wt, nullptr, nullptr, T_out, Y16, DR_HEAD_CIN, 9, Cout, (int)R, H, W, Cout};
    return dr_launch<4, DR_SHIFT, DR_RES>(a, 0, s);
}

extern "C" int sei_drunet_tail(const uint16_t *X, const uint16_t *Wt, int Cin, int B, int H, int W, float *out, void *stream) {
    SEI_REQUIRE(X && Wt && out && dr_al16(X) && dr_al16(Wt) && ((uintptr_t)out & 3) == 0);
    SEI_REQUIRE(dr_width(Cin));
    const long long R = dr_rows(B, H, W);
    SEI_REQUIRE(R > 0);
    DrArgs a{X, Wt, nullptr, nullptr, out, nullptr, Cin, 9, 16, (int)R, H, W, 3};
    return dr_launch<1, DR_SHIFT, DR_TAIL>(a, 0, (hipStream_t)stream);
}
