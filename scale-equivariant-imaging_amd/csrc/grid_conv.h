// grid_conv: the one-wave implicit GEMM over a zero-bordered channels-last grid, the body of drunet_gemm_kernel
// (drunet_kernels.hip) and of adm_conv_kernel (adm_kernels.hip), with the host helpers both families share.
//
// Layout. A convolution's input is a bf16 channels-last grid (B, H + 2, W + 2, C) with a zero border: R = B (H + 2) (W + 2)
// rows with W + 3 guard rows in front and behind (the layout of sei_pad_nhwc_bf16). Results are float32 and / or bf16 on
// the same row indexing. Weights are bf16, tap-major (N, taps * Cin), K-contiguous.
//
// The GEMM is D[n][r] = sum over taps t and channels c of Wt[n][t Cin + c] X[src_t(r)][c], the weights as the MFMA's A
// operand and the grid rows as its B operand, so a lane's four accumulator elements are four neighbouring CHANNELS of one
// grid row (16-byte float32 / 8-byte bf16 stores). Both operands are K-contiguous, so a lane's fragment (8 bf16 of one row)
// is ONE 16-byte global load: no LDS image, no barrier; the loads of two reduction steps ahead are in flight behind a
// step's MFMAs. (The LDS-DMA staged form of gemm_bf16nt.hip is the known next step; DESIGN 4.11 has the measured rates.)
// Every output element is one wave's k-ordered MFMA chain over its own row's inputs: no split-K, no atomics, the same
// bits on every run and wherever the image sits in the batch. The epilogue is called for interior rows only: the border
// of an output grid stays as the caller zeroed it, guard rows are read (into results that are dropped) and never written.
#pragma once
#include "sei_common.h"

namespace {

struct GridConv {
    const uint16_t *X;                       // row 0 of the input grid
    const uint16_t *Wt;                      // (N, ntaps * Cin)
    int Cin, ntaps, N, M;                    // M = rows of the grid the launch walks
    int H, W;                                // interior extents of that grid
};
struct GridRow {
    int row, b, i, j;                        // a grid row (clamped to the last one), its image, grid line and grid column
};

// One wave per workgroup: PB 16-row blocks of grid rows x NB 16-channel blocks. The reduction runs in steps of 32 channels
// of one tap (Cin / 32 steps per tap); a step's fragments are PB + NB 16-byte loads per lane, and the loads of the two
// steps ahead are in flight while a step's MFMAs run (three register sets): with one to six waves per SIMD there is little
// else to hide the L2 latency behind. epilogue(row, n, acc) is called once per (16-row block, 16-channel block) of a lane
// whose row is an interior one: acc[e] is channel n + e of that row.
// DOWN: the taps are the 2x2 patch of a grid of twice the extents (a stride-2 convolution), else the row's 3x3
// neighbourhood (ntaps 9) or the row itself (ntaps 1). POW2: the steps per tap are a power of two and the tap of a step
// is a shift and a mask; else it comes from a multiply and a shift, exact below 2^20 / spt steps.
template <int NB, int PB, bool DOWN, bool POW2, class Epilogue>
__device__ __forceinline__ void grid_conv(const GridConv &a, Epilogue epilogue) {
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
        long long src = mrow[p];             // the row itself, every tap adds its shift
        if (DOWN)                            // tap (0, 0) of the 2x2 patch; a border row reads (and drops) the patch at row 0
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
    const unsigned inv = ((1u << 20) + spt - 1) / spt;
    const int in_w = DOWN ? 2 * a.W + 2 : Wp;
    auto load = [&](int s, bf16x8(&fx)[PB], bf16x8(&fw)[NB]) {
        int t, c0, shift;                    // wave-uniform: the tap, its first channel, grid rows from the base row to it
        if (POW2) t = s >> spt_log2, c0 = (s & (spt - 1)) << 5;
        else t = (int)(((unsigned)s * inv) >> 20), c0 = (s - t * spt) << 5;
        if (DOWN) shift = (t >> 1) * in_w + (t & 1);
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
        for (int j = 0; j < NB; ++j) epilogue(GridRow{mrow[p], bi[p], ii[p], jj[p]}, n0 + 16 * j + 4 * lg, acc[j][p]);
    }
}

// the tail epilogue: channels n .. n + 3 below C of an interior row into the (B, C, H, W) float32 image
__device__ __forceinline__ void grid_store_nchw(float *out, int C, int H, int W, const GridRow &r, int n, const f32x4 &v) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (n + e < C) out[(((size_t)r.b * C + n + e) * H + (r.i - 1)) * W + (r.j - 1)] = v[e];
}

// x (B, 3, H, W) float32 and a constant c3 -> a head's input grid: 32 channels (x, c3, zeros) per row, border rows zero.
// The constant channel is zero on the border like the image, which is why it is no bias.
constexpr int GRID_HEAD_CIN = 32;
__global__ void grid_pack_image_kernel(const float *x, float c3, uint16_t *g, int B, int H, int W) {
    const int Hp = H + 2, Wp = W + 2;
    const size_t n = (size_t)B * Hp * Wp * (GRID_HEAD_CIN / 8);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int chunk = (int)(i % (GRID_HEAD_CIN / 8));
        const size_t r = i / (GRID_HEAD_CIN / 8);
        const int j = (int)(r % Wp), q = (int)(r / Wp), ii = q % Hp, b = q / Hp;
        u32x4 v{0u, 0u, 0u, 0u};
        if (chunk == 0 && ii >= 1 && ii <= H && j >= 1 && j <= W) {
            const size_t plane = (size_t)H * W, at = (size_t)b * 3 * plane + (size_t)(ii - 1) * W + (j - 1);
            v[0] = sei_pack2_bf16(x[at], x[at + plane]);
            v[1] = sei_pack2_bf16(x[at + 2 * plane], c3);
        }
        *reinterpret_cast<u32x4 *>(g + r * GRID_HEAD_CIN + 8 * chunk) = v;
    }
}
void grid_pack_image(const float *x, float c3, uint16_t *g, long long rows, int B, int H, int W, hipStream_t s) {
    hipLaunchKernelGGL(grid_pack_image_kernel, dim3(sei_capped_grid((size_t)rows * (GRID_HEAD_CIN / 8), 256, 4096)), dim3(256), 0,
                       s, x, c3, g, B, H, W);
}

bool grid_al16(const void *p) { return ((uintptr_t)p & 15) == 0; }
// rows of the zero-bordered grid of B images of H x W, 0 when the arguments are refused (or the row count leaves int)
long long grid_rows(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1 || H > 16384 || W > 16384) return 0;
    const long long r = (long long)B * (H + 2) * (W + 2);
    return r < (1ll << 30) ? r : 0;
}

// Grid rows per wave: 16 pb. The measured table (tools/exp_drunet.py): 64 rows win wherever they leave the
// launch 392 waves or more (levels 0 - 2 of a 256 x 384 image and of 32 patches of 48 x 48) and lose to 32 rows at 216 and
// 256 waves (level 3 of either: fewer waves than the chip has CUs); 16 rows never won. So: 64 rows when that gives
// GRID_MIN_WAVES waves, else 32.
constexpr long long GRID_MIN_WAVES = 320;
int grid_default_pb(long long rows, int N, int nb) {
    return (long long)sei_ceil_div((size_t)rows, 64) * (N / (16 * nb)) >= GRID_MIN_WAVES ? 4 : 2;
}
template <int NB, int PB>
dim3 grid_conv_waves(int M, int N) {
    return dim3((unsigned)sei_ceil_div((size_t)M, 16 * PB), (unsigned)(N / (16 * NB)));
}

}  // namespace
