"""Host-side construction of the separable resampling matrices and their band storage.

These are constants of an operator (like the blur taps): computed once in float64 numpy, stored as
float32 band arrays on the device, consumed by `sei_resample_sepband`.

Formulas (restating ATen, as the reference reaches them through F.interpolate):
  * antialiased bicubic (a = -0.5), `_upsample_bicubic2d_aa`: used by Downsampling.A
    (reference src/physics/downsampling/__init__.py:16-19) and the EI antialias pre-filter
    (src/transforms.py:46-57);
  * plain bicubic (a = -0.75, align_corners=False, clamped taps), `upsample_bicubic2d`: the deprecated
    A_adjoint (downsampling/__init__.py:33-34) and the non-antialiased 'normal' transform.
"""
from math import floor

import numpy as np


def _cubic(t, a):
    t = abs(t)
    if t <= 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0
    if t < 2.0:
        return (((t - 5.0) * t + 8.0) * t - 4.0) * a
    return 0.0


def resized_length(n_in, scale_factor):
    """Output length of F.interpolate(scale_factor=...): floor(n_in * scale_factor) in double."""
    return int(floor(float(n_in) * float(scale_factor)))


def aa_bicubic_matrix(n_in, scale_factor):
    """Dense (n_out, n_in) antialiased-bicubic matrix for F.interpolate(scale_factor, antialias=True)."""
    n_out = resized_length(n_in, scale_factor)
    scale = 1.0 / float(scale_factor)
    support = 2.0 * scale if scale >= 1.0 else 2.0
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    m = np.zeros((n_out, n_in))
    for o in range(n_out):
        centre = scale * (o + 0.5)
        first = max(0, int(centre - support + 0.5))
        last = min(n_in, int(centre + support + 0.5))
        w = np.array([_cubic((j - centre + 0.5) * inv, -0.5) for j in range(first, last)])
        m[o, first:last] = w / w.sum()
    return m


def aa_bicubic_matrix_to_size(n_in, n_out):
    """Dense (n_out, n_in) antialiased-bicubic matrix for F.interpolate(size=n_out, antialias=True): as
    aa_bicubic_matrix with the scale ATen derives from the sizes, n_in / n_out (area_pixel_compute_scale with
    align_corners=False and no scale_factor)."""
    scale = float(n_in) / float(n_out)
    support = 2.0 * scale if scale >= 1.0 else 2.0
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    m = np.zeros((n_out, n_in))
    for o in range(n_out):
        centre = scale * (o + 0.5)
        first = max(0, int(centre - support + 0.5))
        last = min(n_in, int(centre + support + 0.5))
        w = np.array([_cubic((j - centre + 0.5) * inv, -0.5) for j in range(first, last)])
        m[o, first:last] = w / w.sum()
    return m


def plain_bicubic_matrix(n_in, scale_factor):
    """Dense (n_out, n_in) matrix of F.interpolate(scale_factor, mode='bicubic') without antialias."""
    n_out = resized_length(n_in, scale_factor)
    scale = 1.0 / float(scale_factor)
    m = np.zeros((n_out, n_in))
    for o in range(n_out):
        src = scale * (o + 0.5) - 0.5
        f = floor(src)
        t = src - f
        co = (_cubic(t + 1.0, -0.75), _cubic(t, -0.75), _cubic(1.0 - t, -0.75), _cubic(2.0 - t, -0.75))
        for d in range(4):
            m[o, min(max(int(f) - 1 + d, 0), n_in - 1)] += co[d]
    return m


def plain_bicubic_matrix_to_size(n_in, n_out):
    """Dense (n_out, n_in) matrix of F.interpolate(size=n_out, mode='bicubic', align_corners=False): as
    plain_bicubic_matrix with the scale ATen derives from the sizes (n_in / n_out)."""
    scale = float(n_in) / float(n_out)
    m = np.zeros((n_out, n_in))
    for o in range(n_out):
        src = scale * (o + 0.5) - 0.5
        f = floor(src)
        t = src - f
        co = (_cubic(t + 1.0, -0.75), _cubic(t, -0.75), _cubic(1.0 - t, -0.75), _cubic(2.0 - t, -0.75))
        for d in range(4):
            m[o, min(max(int(f) - 1 + d, 0), n_in - 1)] += co[d]
    return m


BLUR_PADDINGS = ("circular", "replicate", "reflect", "valid")


def blur_axis_offsets(K):
    """(s, p) of one axis of the legacy Blur with K taps: output i reads positions i - a + s, a in [0, K), of an image
    padded by p on each side. The reference (src/physics/blur/__init__.py:9-62) flips the filter, zero-extends an even
    length by one at the end and a single tap to three, and pads by half the extended length."""
    if K < 1:
        raise ValueError(f"blur: a filter axis needs at least one tap, got {K}")
    if K == 1:
        return 0, 1
    if K % 2:
        return K // 2, K // 2
    return K // 2 - 1, K // 2


def blur_axis_matrix(n, taps, mode):
    """Dense float64 (n_out, n) matrix of one axis of Blur(padding=mode) on an image of length n, literally
    y[i] = sum_a taps[a] x[map(i - a + s)]: map is e mod n (circular), the clamp to [0, n-1] (replicate) or the mirror
    about 0 and n-1 (reflect; needs p <= n-1, as torch's pad does). valid: y[i'] = sum_a taps[a] x[i' + p - a + s] for i'
    in [0, n - 2p), which needs n > 2p. In two dimensions the operator is M_v x M_h^T, its adjoint M_v^T g M_h."""
    c = np.asarray(taps, dtype=np.float64).reshape(-1)
    K = c.size
    s, p = blur_axis_offsets(K)
    if mode not in BLUR_PADDINGS:
        raise ValueError(f"blur: padding must be one of {BLUR_PADDINGS}, got {mode!r}")
    if mode == "valid":
        if n <= 2 * p:
            raise ValueError(f"blur: padding='valid' needs an extent above {2 * p} for a kernel of {K} taps, got {n}")
        m = np.zeros((n - 2 * p, n))
        for i in range(n - 2 * p):
            for a in range(K):
                m[i, i + p - a + s] += c[a]
        return m
    if mode == "reflect" and p > n - 1:
        raise ValueError(f"blur: padding='reflect' pads by {p} for a kernel of {K} taps, which an extent of {n} "
                         f"cannot mirror (it needs an extent of at least {p + 1})")
    m = np.zeros((n, n))
    for i in range(n):
        for a in range(K):
            e = i - a + s
            if mode == "circular":
                e %= n
            elif mode == "replicate":
                e = min(max(e, 0), n - 1)
            else:
                e = -e if e < 0 else 2 * (n - 1) - e if e > n - 1 else e
            m[i, e] += c[a]
    return m


def blur_decimate_axis_matrix(n, taps, mode, rate, phase=0):
    """Dense float64 (n_out, n) matrix of one axis of BlurDownsampling: the rows phase, phase + rate, ... of
    blur_axis_matrix(n, taps, mode), n_out = ceil((n - phase) / rate) -- y[i'] = sum_a taps[a] x[map(rate i' + phase - a + s)].
    `valid` is refused: the image is then not rate times the measurement."""
    if mode == "valid":
        raise ValueError("blur then decimate: padding='valid' is not part of this operator (the image is then not rate "
                         "times the measurement); use circular, replicate or reflect")
    rate, phase = int(rate), int(phase)
    if rate < 1 or not 0 <= phase < rate:
        raise ValueError(f"blur then decimate: needs a rate >= 1 and a phase in [0, rate), got rate {rate}, phase {phase}")
    if phase >= n:
        raise ValueError(f"blur then decimate: phase {phase} leaves no sample of an extent of {n}")
    return np.ascontiguousarray(blur_axis_matrix(n, taps, mode)[phase::rate])


def to_band(dense):
    """Dense (n_out, n_in) -> (weights (n_out, nb) f32, lo (n_out,) i32, nb, max step of lo).
    Band starts are made non-decreasing (a row whose leading weights are exact zeros of the cubic
    simply keeps them inside its band)."""
    n_out, n_in = dense.shape
    lo = np.zeros(n_out, dtype=np.int64)
    hi = np.zeros(n_out, dtype=np.int64)
    for o in range(n_out):
        nz = np.nonzero(dense[o])[0]
        lo[o], hi[o] = (nz[0], nz[-1] + 1) if nz.size else (n_in, 0)
    lo = np.minimum.accumulate(lo[::-1])[::-1]          # running min from the end
    hi = np.maximum.accumulate(hi)                      # running max from the start
    lo = np.minimum(lo, n_in - 1)
    hi = np.maximum(hi, lo + 1)
    nb = int((hi - lo).max())
    w = np.zeros((n_out, nb), dtype=np.float32)
    for o in range(n_out):
        w[o, : hi[o] - lo[o]] = dense[o, lo[o]:hi[o]]
    step = int(np.diff(lo).max()) if n_out > 1 else 0
    return w, lo.astype(np.int32), nb, step
