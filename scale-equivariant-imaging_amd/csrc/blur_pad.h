// The boundary rules of the blur family, shared by physics_kernels.hip (sei_blur_dense_pad) and blur_decimate.hip
// (sei_blur_decimate): the staging index maps, the per-axis offsets of the legacy Blur, the operand overlap test, and the
// launcher of the adjoint's fold (the kernel itself lives in physics_kernels.hip).
#pragma once
#include "sei_common.h"

enum { PAD_CIRCULAR = 0, PAD_REPLICATE = 1, PAD_REFLECT = 2, PAD_VALID = 3, PAD_ZERO = 4 };

template <int MODE>
__device__ __forceinline__ float pad_fetch(const float *__restrict__ xp, int e, int f, int H, int W) {
    if (MODE == PAD_ZERO) return (e >= 0 && e < H && f >= 0 && f < W) ? xp[(size_t)e * W + f] : 0.f;
    if (MODE == PAD_CIRCULAR) return xp[(size_t)sei_mod(e, H) * W + sei_mod(f, W)];     // any number of wraps
    if (MODE == PAD_REFLECT) {
        e = e < 0 ? -e : e;
        e = e > H - 1 ? 2 * (H - 1) - e : e;
        f = f < 0 ? -f : f;
        f = f > W - 1 ? 2 * (W - 1) - f : f;
    }
    // the replicate rule. For the other two it only keeps the halo of a partial last tile inside the plane: their own
    // rule leaves every position that feeds a written output in range already.
    e = min(max(e, 0), H - 1);
    f = min(max(f, 0), W - 1);
    return xp[(size_t)e * W + f];
}

// One axis of K taps reads s positions before its output and K-1-s after it, of an image padded by p: (K/2, K/2) for
// odd K >= 3, (K/2 - 1, K/2) for even K, (0, 1) for K = 1 (sei_hip.h).
static inline void blur_pad_axis(int K, int &s, int &p) {
    if (K == 1) s = 0, p = 1;
    else if (K & 1) s = p = K / 2;
    else s = K / 2 - 1, p = K / 2;
}

static inline bool floats_overlap(const float *a, size_t na, const float *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb * sizeof(float) && b0 < a0 + na * sizeof(float);
}

// physics_kernels.hip: out (planes, H, W) = the fold of the canvas Z (planes, H + 2pv, W + 2ph) under the replicate or
// reflect axis maps (blur_pad_fold_kernel: a gather in a fixed order). Shared between translation units, not exported.
__attribute__((visibility("hidden"))) int sei_blur_pad_fold_launch(int mode, const float *Z, float *out, int planes, int H,
                                                                    int W, int pv, int ph, hipStream_t s);
