// The DRUNet denoiser of the PlugAndPlay baseline (models/drunet.py) for gfx950: a bias-free ResNet-UNet of 3x3
// convolutions at 64 / 128 / 256 / 512 channels, 2x2 stride-2 convolutions down and 2x2 transposed convolutions up.
//
// Layout and kernel body: csrc/grid_conv.h (bf16 channels-last zero-bordered grids with guard rows, the one-wave implicit
// GEMM with fragments straight from global memory). The residual trunk T is float32 on the same row indexing. One
// __global__ template serves the whole family; what a member adds to the shared body is its epilogue.
//
// The network's vector-Jacobian product (models/drunet.py, for the DPS baseline) is the same family with transposed weights
// and one more epilogue, DR_MASK16: Y16 = bf16(conv(X)) where a taped bf16 grid (a ResBlock's ReLU output) is above zero,
// else 0 -- the first half of the block's backward (sei_drunet_conv3x3_masked).
#include "grid_conv.h"

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

// grid_conv with the family's epilogue. (Cin / 32 steps per tap are a power of two here.)
template <int NB, int PB, int GATHER, int EPI>
__global__ __launch_bounds__(64) void drunet_gemm_kernel(const DrArgs a) {
    const GridConv core{a.X, a.Wt, a.Cin, a.ntaps, a.N, a.M, a.H, a.W};
    grid_conv<NB, PB, GATHER == DR_DOWN, true>(core, [&](const GridRow &r, int n, f32x4 v) {
        const size_t at = (size_t)r.row * a.N + n;
        if (EPI == DR_RELU16) {
            *reinterpret_cast<u32x2 *>(a.Y16 + at) =
                u32x2{sei_pack2_bf16(fmaxf(v[0], 0.f), fmaxf(v[1], 0.f)), sei_pack2_bf16(fmaxf(v[2], 0.f), fmaxf(v[3], 0.f))};
        } else if (EPI == DR_MASK16) {                 // the ResBlock's backward: the ReLU's derivative from its taped output
            const u32x2 m = *reinterpret_cast<const u32x2 *>(a.Mask + at);
#pragma unroll
            for (int e = 0; e < 4; ++e)                // a bf16 is above zero when its bits, read as int16, are
                if ((int16_t)(m[e >> 1] >> (16 * (e & 1))) <= 0) v[e] = 0.f;
            *reinterpret_cast<u32x2 *>(a.Y16 + at) = u32x2{sei_pack2_bf16(v[0], v[1]), sei_pack2_bf16(v[2], v[3])};
        } else if (EPI == DR_RES) {
            if (a.Tin) v = *reinterpret_cast<const f32x4 *>(a.Tin + at) + v;
            if (a.Tskip) v = v + *reinterpret_cast<const f32x4 *>(a.Tskip + at);
            *reinterpret_cast<f32x4 *>(a.Tout + at) = v;
            *reinterpret_cast<u32x2 *>(a.Y16 + at) = u32x2{sei_pack2_bf16(v[0], v[1]), sei_pack2_bf16(v[2], v[3])};
        } else if (EPI == DR_UP) {
            const int tap = n / a.Cout, co = n - tap * a.Cout;
            const long long dst = ((long long)r.b * (2 * a.H + 2) + 2 * r.i - 1 + (tap >> 1)) * (2 * a.W + 2) + 2 * r.j - 1 +
                                  (tap & 1);
            const size_t up = (size_t)dst * a.Cout + co;
            *reinterpret_cast<f32x4 *>(a.Tout + up) = v;
            *reinterpret_cast<u32x2 *>(a.Y16 + up) = u32x2{sei_pack2_bf16(v[0], v[1]), sei_pack2_bf16(v[2], v[3])};
        } else {
            grid_store_nchw(a.Tout, a.Cout, a.H, a.W, r, n, v);
        }
    });
}

bool dr_width(int c) { return c == 64 || c == 128 || c == 256 || c == 512; }

template <int NB, int PB, int GATHER, int EPI>
int dr_launch_pb(const DrArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((drunet_gemm_kernel<NB, PB, GATHER, EPI>), (grid_conv_waves<NB, PB>(a.M, a.N)), dim3(64), 0, s, a);
    return sei_launch_status();
}

// (rows per wave: grid_default_pb of grid_conv.h; pb = 1 stays reachable through sei_drunet_conv3x3_ex)
bool dr_pb_ok(int pb) { return pb == 1 || pb == 2 || pb == 4; }
template <int NB, int GATHER, int EPI>
int dr_launch(const DrArgs &a, int pb, hipStream_t s) {
    if (pb == 0) pb = grid_default_pb(a.M, a.N, NB);
    switch (pb) {
        case 1: return dr_launch_pb<NB, 1, GATHER, EPI>(a, s);
        case 2: return dr_launch_pb<NB, 2, GATHER, EPI>(a, s);
        default: return dr_launch_pb<NB, 4, GATHER, EPI>(a, s);
    }
}

}  // namespace

extern "C" size_t sei_drunet_work_bytes(int B, int H, int W) {
    const long long r = grid_rows(B, H, W);
    return r ? (size_t)(r + 2 * (W + 3)) * GRID_HEAD_CIN * sizeof(uint16_t) : 0;
}

extern "C" int sei_drunet_conv3x3_ex(const uint16_t *X, const uint16_t *Wt, int Cin, int Cout, int B, int H, int W,
                                     int epilogue, const float *T_in, const float *T_skip, float *T_out, uint16_t *Y16,
                                     int pb, void *stream) {
    SEI_REQUIRE(pb == 0 || dr_pb_ok(pb));
    SEI_REQUIRE(X && Wt && Y16 && X != Y16 && grid_al16(X) && grid_al16(Wt) && grid_al16(Y16));
    SEI_REQUIRE(dr_width(Cin) && dr_width(Cout) && (epilogue == 0 || epilogue == 1));
    const long long R = grid_rows(B, H, W);
    SEI_REQUIRE(R > 0);
    if (epilogue == 0) SEI_REQUIRE(!T_in && !T_skip && !T_out);
    else SEI_REQUIRE(T_in && T_out && grid_al16(T_in) && grid_al16(T_skip) && grid_al16(T_out));
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
    SEI_REQUIRE(X && Wt && Mask && Y16 && X != Y16 && Mask != Y16 && grid_al16(X) && grid_al16(Wt) && grid_al16(Mask) && grid_al16(Y16));
    SEI_REQUIRE(dr_width(Cin) && dr_width(Cout));
    const long long R = grid_rows(B, H, W);
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
    SEI_REQUIRE(X && Wt && T_out && Y16 && X != Y16 && grid_al16(X) && grid_al16(Wt) && grid_al16(T_out) && grid_al16(Y16));
    SEI_REQUIRE(dr_width(Cin) && dr_width(Cout));
    const long long R = grid_rows(B, Ho, Wo);
    SEI_REQUIRE(R > 0 && grid_rows(B, 2 * Ho, 2 * Wo) > 0);
    DrArgs a{X, Wt, nullptr, nullptr, T_out, Y16, Cin, 4, Cout, (int)R, Ho, Wo, Cout};
    return dr_launch<4, DR_DOWN, DR_RES>(a, 0, (hipStream_t)stream);
}

extern "C" int sei_drunet_up(const uint16_t *X, const uint16_t *Wt, int Cin, int Cout, int B, int H, int W, float *T_out,
                             uint16_t *Y16, void *stream) {
    SEI_REQUIRE(X && Wt && T_out && Y16 && X != Y16 && grid_al16(X) && grid_al16(Wt) && grid_al16(T_out) && grid_al16(Y16));
    SEI_REQUIRE(dr_width(Cin) && dr_width(Cout));
    const long long R = grid_rows(B, H, W);
    SEI_REQUIRE(R > 0 && grid_rows(B, 2 * H, 2 * W) > 0);
    DrArgs a{X, Wt, nullptr, nullptr, T_out, Y16, Cin, 1, 4 * Cout, (int)R, H, W, Cout};
    return dr_launch<4, DR_SHIFT, DR_UP>(a, 0, (hipStream_t)stream);
}

extern "C" int sei_drunet_head(const float *x, float sigma, const uint16_t *Wt, int Cout, int B, int H, int W, float *T_out,
                               uint16_t *Y16, void *work, void *stream) {
    SEI_REQUIRE(x && Wt && T_out && Y16 && work && ((uintptr_t)x & 3) == 0 && grid_al16(Wt) && grid_al16(T_out) &&
                grid_al16(Y16) && grid_al16(work));
    SEI_REQUIRE(dr_width(Cout) && sigma == sigma);
    const long long R = grid_rows(B, H, W);
    SEI_REQUIRE(R > 0);
    hipStream_t s = (hipStream_t)stream;
    uint16_t *grid = reinterpret_cast<uint16_t *>(work) + (size_t)(W + 3) * GRID_HEAD_CIN;
    grid_pack_image(x, sigma, grid, R, B, H, W, s);          // channel 3: the noise level
    DrArgs a{grid, Wt, nullptr, nullptr, T_out, Y16, GRID_HEAD_CIN, 9, Cout, (int)R, H, W, Cout};
    return dr_launch<4, DR_SHIFT, DR_RES>(a, 0, s);
}

extern "C" int sei_drunet_tail(const uint16_t *X, const uint16_t *Wt, int Cin, int B, int H, int W, float *out, void *stream) {
    SEI_REQUIRE(X && Wt && out && grid_al16(X) && grid_al16(Wt) && ((uintptr_t)out & 3) == 0);
    SEI_REQUIRE(dr_width(Cin));
    const long long R = grid_rows(B, H, W);
    SEI_REQUIRE(R > 0);
    DrArgs a{X, Wt, nullptr, nullptr, out, nullptr, Cin, 9, 16, (int)R, H, W, 3};
    return dr_launch<1, DR_SHIFT, DR_TAIL>(a, 0, (hipStream_t)stream);
}
