"""The noise estimator of include/sei_hip.h (sei_noise_quad_hist, sei_noise_fit) restated in numpy: the histogram in
float32, one rounding per operation and in the header's order; the fit in float64 Python scalars, sequential loops in index
order. Every pin of tests/test_noise_estimation*.py is against this file. Also the synthetic measurement both test files
share (piecewise-constant rectangles plus low-frequency sinusoids, circularly blurred)."""
import math

import numpy as np

LEVELS, BINS, LATTICE = 64, 256, 510
C_MAD = 0.6744897501960817
LEVEL_LO, LEVEL_HI, N_MIN = 6, 57, 256
FLAG_EMPTY, FLAG_POOLED_OVERFLOW, FLAG_NO_LINE, FLAG_NEGATIVE_SLOPE, FLAG_NEGATIVE_INTERCEPT = 1, 2, 4, 8, 16

f32 = np.float32


def quad_hist(y, hist=None):
    """y: (..., H, W) float32 array -> (64, 256) uint64 counts, added to `hist` when given."""
    y = np.asarray(y)
    assert y.dtype == np.float32 and y.ndim >= 2
    H, W = y.shape[-2:]
    y = y.reshape(-1, H, W)[:, :H // 2 * 2, :W // 2 * 2]
    a, b, c, d = y[:, 0::2, 0::2], y[:, 0::2, 1::2], y[:, 1::2, 0::2], y[:, 1::2, 1::2]
    ok = np.ones(a.shape, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in (a, b, c, d):
            ok &= (p > 0) & (p < 1)                      # (False for NaN)
        s = ((a + b) + (c + d)) * f32(0.25)
        t = ((a - b) - (c - d)) * f32(0.5)
        assert s.dtype == np.float32 and t.dtype == np.float32
        s, t = s[ok], t[ok]
        lvl = np.clip(np.floor(s * f32(64.0)).astype(np.int64), 0, LEVELS - 1)
        scaled = np.abs(t) * f32(510.0)                  # rounded to float32 here,
        k = np.minimum(BINS - 1, np.floor(scaled + f32(0.5)).astype(np.int64))      # ... and again after the sum
    out = np.zeros((LEVELS, BINS), dtype=np.uint64) if hist is None else hist.copy()
    np.add.at(out, (lvl, k), np.uint64(1))
    return out


def median(h):
    """(interpolated median of the K-bin row h in signal units, its bin); the row's total must be positive."""
    h = [int(v) for v in h]
    n = sum(h)
    assert n > 0
    half = n / 2
    below, j = 0, 0
    while j < BINS - 1 and below + h[j] < half:
        below += h[j]
        j += 1
    lo, hi = max(j - 0.5, 0.0), j + 0.5
    return (lo + (hi - lo) * (half - below) / h[j]) / LATTICE, j


def fit(hist):
    """(64, 256) counts -> [sigma, eta, gamma, levels_used, quads_counted, flags, 0, 0] as Python floats."""
    hist = np.asarray(hist).astype(np.uint64).reshape(LEVELS, BINS)
    rows = [[int(v) for v in hist[l]] for l in range(LEVELS)]
    pooled = [sum(rows[l][k] for l in range(LEVELS)) for k in range(BINS)]
    n = sum(pooled)
    nan = math.nan
    if n == 0:
        return [nan, nan, nan, 0.0, 0.0, float(FLAG_EMPTY), 0.0, 0.0]
    flags = 0
    med, j = median(pooled)
    sigma = med / C_MAD
    if j == BINS - 1:
        sigma, flags = nan, flags | FLAG_POOLED_OVERFLOW
    used = []
    sw = swm = swv = swmm = swmv = 0.0
    for l in range(LEVEL_LO, LEVEL_HI + 1):
        nl = sum(rows[l])
        if nl < N_MIN:
            continue
        med, j = median(rows[l])
        if j == BINS - 1:
            continue
        q = med / C_MAD
        w, m, v = float(nl), (l + 0.5) / 64.0, q * q
        used.append((w, m, v))
        sw += w
        swm += w * m
        swv += w * v
        swmm += w * m * m
        swmv += w * m * v
    cmm = cmv = 0.0
    if len(used) >= 2:
        mbar, vbar = swm / sw, swv / sw
        for w, m, v in used:
            dm, dv = m - mbar, v - vbar
            cmm += w * dm * dm
            cmv += w * dm * dv
    if len(used) < 2 or not cmm > 0.0:
        gamma, eta, flags = 0.0, sigma * sigma, flags | FLAG_NO_LINE
    else:
        gamma = cmv / cmm
        eta = vbar - gamma * mbar
        if gamma < 0.0:
            gamma, eta, flags = 0.0, vbar, flags | FLAG_NEGATIVE_SLOPE
        elif eta < 0.0:
            eta, gamma, flags = 0.0, swmv / swmm, flags | FLAG_NEGATIVE_INTERCEPT
    return [sigma, eta, gamma, float(len(used)), float(n), float(flags), 0.0, 0.0]


def estimate(y):
    return fit(quad_hist(np.asarray(y, dtype=np.float32)))


# ------------------------------------------------------------------------------------------------ the shared measurement
def clean_image(C=3, H=256, W=256, seed=0):
    """Piecewise-constant rectangles plus low-frequency sinusoids in about [0.08, 0.92], float64 (C, H, W)."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    x = np.empty((C, H, W))
    for c in range(C):
        base = np.full((H, W), 0.5)
        for _ in range(40):
            h0, w0 = rng.integers(0, H), rng.integers(0, W)
            hh, ww = rng.integers(H // 16, H // 2), rng.integers(W // 16, W // 2)
            base[h0:h0 + hh, w0:w0 + ww] = rng.uniform(0.12, 0.88)
        wave = 0.04 * np.sin(2 * np.pi * (i / rng.uniform(48, 96) + rng.uniform())) \
            * np.cos(2 * np.pi * (j / rng.uniform(48, 96) + rng.uniform()))
        x[c] = base + wave
    return x


def gaussian_taps(std=1.5, radius=6):
    g = np.exp(-0.5 * (np.arange(-radius, radius + 1) / std) ** 2)
    return g / g.sum()


def circular_blur(x, std=1.5):
    """Separable circular Gaussian blur of the last two axes, float64."""
    g = gaussian_taps(std)
    r = len(g) // 2
    out = x
    for axis in (-2, -1):
        out = sum(t * np.roll(out, k - r, axis=axis) for k, t in enumerate(g))
    return out


def measure(Ax, sigma, gain, seed, quantise):
    """Gaussian (gain = 0) or Poisson-Gaussian noise on A x, then optionally 8-bit quantisation and clipping, float32."""
    rng = np.random.default_rng(seed)
    y = Ax if gain == 0 else gain * rng.poisson(np.clip(Ax, 0, None) / gain)
    y = y + sigma * rng.standard_normal(Ax.shape)
    if quantise:
        y = np.clip(np.round(y * 255.0), 0, 255) / 255.0
    return y.astype(np.float32)


GAUSSIAN_CASES = (5 / 255, 10 / 255)
PG_CASES = ((2 / 255, 0.01), (5 / 255, 0.003))


def hold_gaussian(name, est, sigma):
    """The issue's condition on a Gaussian case: sigma within 5 % of the truth. Prints before it asserts."""
    dev = est[0] / sigma - 1
    print(f"{name}: sigma {255 * est[0]:.4f} / 255 against {255 * sigma:.4f} / 255 ({100 * dev:+.2f} %), flags {int(est[5])}")
    assert abs(dev) <= 0.05


def hold_poisson_gaussian(name, est, sigma, gain):
    """The issue's conditions on a Poisson-Gaussian case: the variance at signal 0.5 within 10 %, the gain within 25 %."""
    truth = sigma ** 2 + 0.5 * gain
    dev_v = (est[1] + 0.5 * est[2]) / truth - 1
    dev_g = est[2] / gain - 1
    print(f"{name}: eta {est[1]:.3e} gain {est[2]:.5f} against {sigma ** 2:.3e} {gain:.5f}; variance at 0.5 "
          f"{100 * dev_v:+.2f} %, gain {100 * dev_g:+.2f} %, levels {int(est[3])}, flags {int(est[5])}")
    assert abs(dev_v) <= 0.10
    assert abs(dev_g) <= 0.25
