"""The float64 restatement of the BM3D deblurring baseline (models/bm3d.py documents the algorithm): literal and slow, one
plane at a time, numpy for the block work and torch.fft for the two inversions (it keeps float32 where asked). Every function
takes a `dtype` (numpy float64 or float32) and does all of its arithmetic in it, so the restatement can also be run in
float32 on the CPU: the end-to-end test bounds the legitimate divergence of decisions by the restatement against itself in
the two precisions, never by the code under test.

It also reports how close its own run came to a decision:
- match_ref: per reference block, the smallest relative gap (b - a) / b between consecutive sorted distances a <= b among
  the kept ones, across the n_max cut, and |d - tau| / tau at the tau cut;
- ht_ref: per group, the smallest | |c| - threshold | / threshold over its coefficients."""
import numpy as np
import torch

BLOCK = 8
TAU_HT, TAU_WIENER = 3000 / 255 ** 2, 400 / 255 ** 2
N_MAX_HT, N_MAX_WIENER = 16, 32
LAMBDA_3D = 2.7
REG_INVERSE, REG_WIENER = 4e-4, 5e-3
TINY = 1e-300


def dct_matrix(dtype=np.float64):
    """D[j, m] = c_j cos(pi (2 m + 1) j / 16): the orthonormal 8-point DCT-II, coefficients = D x."""
    j, m = np.arange(BLOCK)[:, None], np.arange(BLOCK)[None, :]
    D = np.sqrt(2.0 / BLOCK) * np.cos(np.pi * (2 * m + 1) * j / (2 * BLOCK))
    D[0] /= np.sqrt(2.0)
    return D.astype(dtype)


def haar(x, inverse=False):
    """The full orthonormal Haar decomposition along axis 0 (a power-of-two length): pairs (a + b) / sqrt 2 and
    (a - b) / sqrt 2 at stride 1, then the same on the sums (which sit at the even multiples of the stride) at stride 2, 4,
    ...; in place, so the sums of stride s end at the multiples of 2 s. The butterfly is its own inverse: the inverse runs
    the strides backwards."""
    x = np.array(x, copy=True)
    n = x.shape[0]
    assert n >= 1 and n & (n - 1) == 0
    r = x.dtype.type(np.sqrt(0.5))
    strides = []
    s = 1
    while s < n:
        strides.append(s)
        s *= 2
    for s in (reversed(strides) if inverse else strides):
        a, b = x[0::2 * s].copy(), x[s::2 * s].copy()
        x[0::2 * s], x[s::2 * s] = (a + b) * r, (a - b) * r
    return x


def haar_matrix(n, dtype=np.float64):
    return haar(np.eye(n, dtype=dtype))


def positions(m, step=3):
    """Reference positions along an axis of extent m: 0, step, 2 step ... up to m - 8, and m - 8 itself if missed."""
    p = list(range(0, m - BLOCK + 1, step))
    if p[-1] != m - BLOCK:
        p.append(m - BLOCK)
    return p


def kaiser_window(dtype=np.float64):
    k = np.kaiser(BLOCK, 2.0)
    return np.outer(k, k).astype(dtype)


def _torch_dtype(dtype):
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def otf_ref(kernel, H, W, dtype=np.float64):
    """The unnormalised fft2 of the kernel zero-padded to H x W with its centre (kh // 2, kw // 2) rolled to the origin
    (taps that do not fit wrap around). A complex torch tensor of the precision of `dtype`."""
    k = np.asarray(kernel, dtype=np.float64).reshape(kernel.shape[-2], kernel.shape[-1])
    psf = np.zeros((H, W), dtype=np.float64)
    for i in range(k.shape[0]):
        for j in range(k.shape[1]):
            psf[(i - k.shape[0] // 2) % H, (j - k.shape[1] // 2) % W] += k[i, j]
    return torch.fft.fft2(torch.from_numpy(psf.astype(dtype)))


def coefficient_variances_ref(S, dtype=np.float64):
    """v_(p, q) = (1 / n) sum_xi S(xi) |Psi_(p, q)(xi)|^2 for the 64 DCT basis functions, each zero-padded to H x W: the
    basis is separable, so |Psi|^2 is an outer product and v = A S B^T / n with A[p] = |fft(d_p, H)|^2, B[q] = |fft(d_q, W)|^2."""
    S = np.asarray(S, dtype=dtype)
    H, W = S.shape
    D = torch.from_numpy(dct_matrix(dtype))
    A = (torch.fft.fft(D, n=H, dim=1).abs() ** 2).numpy().astype(dtype)
    B = (torch.fft.fft(D, n=W, dim=1).abs() ** 2).numpy().astype(dtype)
    return ((A @ S @ B.T) / dtype(H * W)).astype(dtype).reshape(64)


def _pow2_floor(n):
    return 1 << (int(n).bit_length() - 1)


def match_ref(img, tau, n_max, step=3, window=39, dtype=np.float64):
    """Groups of one plane. Returns (pos, counts, dists, gaps, before_cut): pos (refs, n_max, 2) int32 with the reference
    position in the unused slots, counts (refs,) int32, dists (refs, n_max) with +inf in the unused slots, gaps (refs,) as
    described in the module docstring, before_cut (refs,) the number kept before the cut to a power of two. Reference blocks
    are row-major over (row position, column position)."""
    img = np.asarray(img, dtype=dtype)
    H, W = img.shape
    half = window // 2
    blocks = np.lib.stride_tricks.sliding_window_view(img, (BLOCK, BLOCK))
    tau = dtype(tau)
    rows, cols = positions(H, step), positions(W, step)
    refs = len(rows) * len(cols)
    pos = np.zeros((refs, n_max, 2), dtype=np.int32)
    counts = np.zeros(refs, dtype=np.int32)
    dists = np.full((refs, n_max), np.inf, dtype=dtype)
    gaps = np.full(refs, np.inf, dtype=np.float64)
    before_cut = np.zeros(refs, dtype=np.int32)
    g = 0
    for r in rows:
        for c in cols:
            rlo, rhi, clo, chi = max(0, r - half), min(H - BLOCK, r + half), max(0, c - half), min(W - BLOCK, c + half)
            diff = blocks[rlo:rhi + 1, clo:chi + 1] - blocks[r, c]
            d = ((diff * diff).reshape(diff.shape[0], diff.shape[1], 64).sum(-1, dtype=dtype) / dtype(64)).reshape(-1)
            order = np.argsort(d, kind="stable")                       # (d, r', c'): candidates are row-major
            ds = d[order]
            kept = int((ds <= tau).sum())
            m = min(kept, n_max)
            count = _pow2_floor(m)
            width = chi - clo + 1
            sel = order[:count]
            pos[g, :, 0], pos[g, :, 1] = r, c
            pos[g, :count, 0], pos[g, :count, 1] = rlo + sel // width, clo + sel % width
            counts[g] = count
            dists[g, :count] = ds[:count]
            # how close the run came to another decision
            dd = ds.astype(np.float64)
            gap = np.inf
            if m > 1:
                gap = min(gap, float(((dd[1:m] - dd[:m - 1]) / np.maximum(dd[1:m], TINY)).min()))
            if kept > n_max:
                gap = min(gap, float((dd[n_max] - dd[n_max - 1]) / max(dd[n_max], TINY)))
            t = max(float(tau), TINY)
            if kept > 0:
                gap = min(gap, (t - dd[kept - 1]) / t if dd[kept - 1] > 0 else np.inf)   # (d = 0 is exact in any precision)
            if kept < len(dd):
                gap = min(gap, (dd[kept] - t) / max(dd[kept], TINY))
            gaps[g] = gap
            before_cut[g] = m
            g += 1
    return pos, counts, dists, gaps, before_cut


def _gather(plane, pos, n):
    return np.stack([plane[r:r + BLOCK, c:c + BLOCK] for r, c in pos[:n]])


def _forward(blocks, D):
    """(N, 8, 8) -> (N, 64) coefficients of the 3-D transform: D B D^T on every block, Haar along the group."""
    return haar(np.einsum("pi,nij,qj->npq", D, blocks, D).reshape(blocks.shape[0], 64))


def _inverse(coef, D):
    return np.einsum("pi,npq,qj->nij", D, haar(coef, inverse=True).reshape(-1, BLOCK, BLOCK), D)


def _aggregate(num, den, est, pos, w, K):
    for k in range(est.shape[0]):
        r, c = pos[k]
        num[r:r + BLOCK, c:c + BLOCK] += w * K * est[k]
        den[r:r + BLOCK, c:c + BLOCK] += w * K


def ht_ref(noisy, var, pos, counts, lambd=LAMBDA_3D, dtype=np.float64):
    """The hard-thresholding stage of one plane on given groups. Returns (out, margins, coefs): margins (refs,) the smallest
    | |c| - threshold | / threshold of each group (inf at lambd = 0), coefs (refs, n_max, 64) the transform coefficients
    before the shrinkage (zeros behind the count)."""
    noisy, var = np.asarray(noisy, dtype=dtype), np.asarray(var, dtype=dtype).reshape(64)
    D, K = dct_matrix(dtype), kaiser_window(dtype)
    thr = dtype(lambd) * np.sqrt(var)
    num, den = np.zeros_like(noisy), np.zeros_like(noisy)
    margins = np.full(len(counts), np.inf)
    coefs = np.zeros((len(counts), pos.shape[1], 64), dtype=dtype)
    for g, n in enumerate(counts):
        C = _forward(_gather(noisy, pos[g], n), D)
        coefs[g, :n] = C
        keep = np.abs(C) > thr
        if lambd > 0:
            margins[g] = float((np.abs(np.abs(C) - thr) / thr).min())
        total = (keep * var).sum(dtype=dtype)
        w = dtype(1) / total if total > 0 else dtype(1)
        _aggregate(num, den, _inverse(np.where(keep, C, dtype(0)), D), pos[g], w, K)
    return num / den, margins, coefs


def wiener_ref(noisy, pilot, var, pos, counts, dtype=np.float64):
    """The Wiener stage of one plane on given groups."""
    noisy, pilot = np.asarray(noisy, dtype=dtype), np.asarray(pilot, dtype=dtype)
    var = np.asarray(var, dtype=dtype).reshape(64)
    D, K = dct_matrix(dtype), kaiser_window(dtype)
    num, den = np.zeros_like(noisy), np.zeros_like(noisy)
    for g, n in enumerate(counts):
        C, P = _forward(_gather(noisy, pos[g], n), D), _forward(_gather(pilot, pos[g], n), D)
        q = P * P + var
        Wc = np.where(q > 0, P * P / np.where(q > 0, q, dtype(1)), dtype(0))
        total = (Wc * Wc * var).sum(dtype=dtype)
        w = dtype(1) / total if total > 0 else dtype(1)
        _aggregate(num, den, _inverse(C * Wc, D), pos[g], w, K)
    return num / den


def inverse_ref(z, V, s2, pilot=None, dtype=np.float64):
    """Step 1 (pilot None) or step 3 of one plane: (the regularised inverse of z, its noise spectrum S)."""
    zt = torch.from_numpy(np.asarray(z, dtype=dtype))
    n = zt.numel()
    V2 = V.real ** 2 + V.imag ** 2
    if pilot is None:
        G = V.conj() / (V2 + REG_INVERSE * s2 * n)
    else:
        Pf = torch.fft.fft2(torch.from_numpy(np.asarray(pilot, dtype=dtype)))
        P2 = Pf.real ** 2 + Pf.imag ** 2
        G = V.conj() * P2 / (P2 * V2 + REG_WIENER * s2 * n)
    out = torch.fft.ifft2(torch.fft.fft2(zt) * G).real
    S = s2 * (G.real ** 2 + G.imag ** 2)
    return out.numpy().astype(dtype), S.numpy().astype(dtype)


def deblur_ref(z, kernel, sigma_psd, dtype=np.float64, step=3, window=39):
    """The four steps on one plane. Returns a dict of every intermediate: z1, S1, v1, groups1 (match_ref's tuple), pilot,
    margins, z2, S2, v2, groups2, out."""
    if not sigma_psd > 0:
        raise ValueError("sigma_psd must be positive")
    z = np.asarray(z, dtype=dtype)
    H, W = z.shape
    s2 = float(sigma_psd) ** 2
    V = otf_ref(kernel, H, W, dtype)
    t = {}
    t["z1"], t["S1"] = inverse_ref(z, V, s2, None, dtype)
    t["v1"] = coefficient_variances_ref(t["S1"], dtype)
    t["groups1"] = match_ref(t["z1"], TAU_HT, N_MAX_HT, step, window, dtype)
    t["pilot"], t["margins"], _ = ht_ref(t["z1"], t["v1"], t["groups1"][0], t["groups1"][1], LAMBDA_3D, dtype)
    t["z2"], t["S2"] = inverse_ref(z, V, s2, t["pilot"], dtype)
    t["v2"] = coefficient_variances_ref(t["S2"], dtype)
    t["groups2"] = match_ref(t["pilot"], TAU_WIENER, N_MAX_WIENER, step, window, dtype)
    t["out"] = wiener_ref(t["z2"], t["pilot"], t["v2"], t["groups2"][0], t["groups2"][1], dtype)
    return t


def edged_image(H, W, seed, planes=1, edges=3, steep=40.0):
    """Two low-frequency cosines and `edges` steep straight edges per plane, in [0.1, 0.9]: what a blur damages most and a
    deblurring method can win back. (planes, H, W) float64."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((planes, H, W))
    for p in range(planes):
        im = np.zeros((H, W))
        for _ in range(2):
            fy, fx, ph = rng.uniform(0.2, 1.0, 2).tolist() + [rng.uniform(0, 2 * np.pi)]
            im += 0.5 * rng.uniform(0.3, 1.0) * np.cos(2 * np.pi * (fy * y / H + fx * x / W) + ph)
        for _ in range(edges):
            a, b, c0, c1 = rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8)
            im += 1.0 * np.tanh((a * (y / H - c0) + b * (x / W - c1)) * steep)
        im -= im.min()
        out[p] = 0.1 + 0.8 * im / im.max()
    return out


def smooth_image(H, W, seed, planes=1):
    """A smooth synthetic image in [0, 1]: a few low-frequency cosines and a soft edge per plane. (planes, H, W) float64."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((planes, H, W))
    for p in range(planes):
        im = np.zeros((H, W))
        for _ in range(4):
            fy, fx, ph = rng.uniform(0.2, 1.5, 2).tolist() + [rng.uniform(0, 2 * np.pi)]
            im += rng.uniform(0.3, 1.0) * np.cos(2 * np.pi * (fy * y / H + fx * x / W) + ph)
        a, b, c0 = rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0.3, 0.7)
        im += 1.5 * np.tanh((a * (y / H - c0) + b * (x / W - c0)) * 12)
        im -= im.min()
        out[p] = 0.1 + 0.8 * im / im.max()
    return out
