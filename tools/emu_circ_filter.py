#!/usr/bin/env python3
"""CPU emulation of circ_filter_sep_kernel (csrc/physics_kernels.hip): the kernel's LDS layout, index arithmetic and
accumulation order restated thread by thread in numpy, with every LDS access checked against the region it belongs to
and LDS poisoned with NaN before each fill. Shows that no index leaves its region and that no unwritten word is read
for odd, non-multiple-of-32 and unit extents, and prints the max-norm relative error against the float64 dense
circulants (a float32 FMA is emulated as one rounding of the float64 product-sum). No GPU needed.

    python tools/emu_circ_filter.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))

from physics._circulant import dense, first_column  # noqa: E402

THREADS, STRIP, ROWS = 256, 32, 32              # CF_THREADS, CF_STRIP, CF_ROWS
SHAPES = [(1, 5), (5, 1), (19, 23), (47, 33), (48, 48), (33, 70), (8, 64), (3, 100)]


def stride(n4):
    """cf_stride: n4 + 4 or n4 + 8, whichever is 4 x odd."""
    return n4 + (8 if (n4 >> 2) & 1 else 4)


def load4(lds, offset, region):
    lo, hi = region
    assert lo <= offset and offset + 4 <= hi, (offset, region)
    return lds[offset:offset + 4]


def cf_dot(outputs, lds, src, n4, taps, tb, src_region, taps_region):
    """cf_dot<outputs>: out[k] = sum_j lds[src + j] * lds[taps + tb + k - j], four partial sums per output."""
    assert src % 4 == 0 and taps % 4 == 0 and tb % 4 == 0 and n4 % 4 == 0
    acc = np.zeros((outputs, 4), np.float32)
    window = np.zeros(outputs + 4, np.float32)
    for q in range(outputs // 4):
        window[4 + 4 * q:8 + 4 * q] = load4(lds, taps + tb + 4 * q, taps_region)
    for jb in range(0, n4, 4):
        window[0:4] = load4(lds, taps + tb - jb - 4, taps_region)
        xv = load4(lds, src + jb, src_region)
        for jj in range(4):
            for k in range(outputs):
                fma = np.float64(xv[jj]) * np.float64(window[4 + k - jj]) + np.float64(acc[k, jj])
                acc[k, jj] = np.float32(fma)
        window[4:] = window[:-4].copy()
    return (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])


def run(x, cv, ch):
    """One plane through every workgroup (strip) of the kernel."""
    H, W = x.shape
    y = np.full((H, W), np.nan, np.float32)
    H4, W4 = (H + 3) & ~3, (W + 3) & ~3
    len_h = ((W + STRIP - 1) & ~(STRIP - 1)) + W4
    len_v = ((H + 7) & ~7) + H4
    xs, ts = stride(W4), stride(H4)
    o_th, o_tv = 0, len_h
    o_x = o_tv + len_v
    o_t = o_x + ROWS * xs
    total = o_t + STRIP * ts
    for strip in range((W + STRIP - 1) // STRIP):
        c0 = STRIP * strip
        lds = np.full(total, np.nan, np.float32)
        for m in range(len_h):
            lds[o_th + m] = ch[(m - W4) % W]
        for m in range(len_v):
            lds[o_tv + m] = cv[(m - H4) % H]
        for r0 in range(0, H4, ROWS):                                   # row pass, a chunk of rows at a time
            lds[o_x:o_t] = np.nan
            for r in range(ROWS):
                i = r0 + r
                for j in range(W4):
                    lds[o_x + r * xs + j] = x[i, j] if (i < H and j < W) else 0
            for tid in range(THREADS):
                rr, cq = tid & 31, 4 * (tid >> 5)
                i = r0 + rr
                if i < H4 and c0 + cq < W:
                    out = np.zeros(4, np.float32)
                    if i < H:
                        row = o_x + rr * xs
                        out = cf_dot(4, lds, row, W4, o_th, c0 + cq + W4, (row, row + W4), (o_th, o_tv))
                    for k in range(4):
                        at = o_t + (cq + k) * ts + i
                        assert o_t <= at < total
                        lds[at] = out[k]
        for tid in range(THREADS):                                      # column pass
            c = tid & 31
            if c0 + c < W:
                for ib in range(tid >> 5, (H + 7) >> 3, THREADS // 32):
                    col = o_t + c * ts
                    out = cf_dot(8, lds, col, H4, o_tv, 8 * ib + H4, (col, col + H4), (o_tv, o_x))
                    for k in range(8):
                        if 8 * ib + k < H:
                            y[8 * ib + k, c0 + c] = out[k]
    return y


def main():
    rng = np.random.default_rng(0)
    for H, W in SHAPES:
        for inverse in (True, False):
            x = rng.random((H, W)).astype(np.float32)
            cv = first_column(H, inverse).astype(np.float32)
            ch = first_column(W, inverse).astype(np.float32)
            y = run(x, cv, ch)
            ref = dense(H, inverse) @ x.astype(np.float64) @ dense(W, inverse).T
            assert not np.isnan(y).any()
            print(f"{H:3d} x {W:3d} inverse={inverse}: {np.abs(y - ref).max() / np.abs(ref).max():.2e}")


if __name__ == "__main__":
    main()
