// The bicubic (A = -0.75) gather with reflection that the EI scale transform (physics_kernels.hip) and the equivariant
// bootstrap (bootstrap_kernels.hip) share: ATen's grid_sampler with mode='bicubic', padding_mode='reflection',
// align_corners=True, from a normalised sampling position on. The coordinate arithmetic is written with the __f*_rn
// intrinsics so that no contraction to FMA can move a sampling position off torch's float32 value.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float cubic1(float x) {   // |x| <= 1, A = -0.75
    const float A = -0.75f;
    return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
}
__device__ __forceinline__ float cubic2(float x) {   // 1 < |x| < 2
    const float A = -0.75f;
    return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
}
__device__ __forceinline__ int reflect_clip(int v, int n) {
    // reflect_coordinates(v, 0, 2(n-1)) then clip, on an integer tap position
    if (n == 1) return 0;
    const int span = n - 1;
    v = v < 0 ? -v : v;
    const int flips = v / span;
    const int extra = v - flips * span;
    const int r = (flips & 1) ? span - extra : extra;
    return min(max(r, 0), n - 1);
}

struct ScaleTaps {
    int xs[4], ys[4];
    float wx[4], wy[4];
};

// taps of the normalised position (gx, gy) in [-1, 1]^2 on an image of Hi rows and Wi columns
__device__ __forceinline__ void bicubic_taps(float gx, float gy, int Hi, int Wi, ScaleTaps &tp) {
    const float ix = __fmul_rn(__fdiv_rn(__fadd_rn(gx, 1.f), 2.f), (float)(Wi - 1));
    const float iy = __fmul_rn(__fdiv_rn(__fadd_rn(gy, 1.f), 2.f), (float)(Hi - 1));
    const float fx = floorf(ix), fy = floorf(iy);
    const float tx = ix - fx, ty = iy - fy;
    tp.wx[0] = cubic2(tx + 1.f); tp.wx[1] = cubic1(tx); tp.wx[2] = cubic1(1.f - tx); tp.wx[3] = cubic2(2.f - tx);
    tp.wy[0] = cubic2(ty + 1.f); tp.wy[1] = cubic1(ty); tp.wy[2] = cubic1(1.f - ty); tp.wy[3] = cubic2(2.f - ty);
    // clamp before the int conversion: far-out-of-range coordinates only arise from absurd rates
    const int bx = (int)fminf(fmaxf(fx, -1.0e8f), 1.0e8f), by = (int)fminf(fmaxf(fy, -1.0e8f), 1.0e8f);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        tp.xs[d] = reflect_clip(bx - 1 + d, Wi);
        tp.ys[d] = reflect_clip(by - 1 + d, Hi);
    }
}

// the weighted sum of the 4 x 4 taps of one plane: rows inner (x first), then the column of row sums
__device__ __forceinline__ float bicubic_gather(const float *__restrict__ xp, int Wi, const ScaleTaps &tp) {
    float acc = 0.f;
#pragma unroll
    for (int dy = 0; dy < 4; ++dy) {
        const float *row = xp + (size_t)tp.ys[dy] * Wi;
        float r = tp.wx[0] * row[tp.xs[0]];
        r = fmaf(tp.wx[1], row[tp.xs[1]], r);
        r = fmaf(tp.wx[2], row[tp.xs[2]], r);
        r = fmaf(tp.wx[3], row[tp.xs[3]], r);
        acc = fmaf(tp.wy[dy], r, acc);
    }
    return acc;
}
