"""Float64 model of the blur-then-decimate operator (physics.BlurDownsampling) on the host, shared by
tests/test_blur_decimate.py and tests/test_blur_decimate_gpu.py: the image padded with the boundary (gathered by index, which
is F.pad where F.pad applies -- tests/test_blur_decimate.py checks that -- and goes on where a circular kernel wraps more
than once), then F.conv2d with stride = rate on the padded image cut at the phase, and its autograd for the transpose.
Written from the operator's definition, not from the package's matrices."""
import numpy as np
import torch
import torch.nn.functional as F


def relerr(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def axis_offsets(K, rule):
    """(s, p) of one axis: output i reads i - a + s of an image padded by p. rule 'v2': BlurV2's circular one, s = K/2;
    'legacy': the reference Blur's (the filter flipped, an even length zero-extended by one, a single tap to three)."""
    if rule == "v2":
        return K // 2, K - 1                      # (any p >= max(s, K-1-s) does)
    if K == 1:
        return 0, 1
    return (K // 2, K // 2) if K % 2 else (K // 2 - 1, K // 2)


def pad_axis_index(n, p, padding):
    """The source pixel of every position -p .. n-1+p of one padded axis, any p (torch's F.pad refuses p >= n for circular
    and reflect; the operator's rule does not stop there for circular)."""
    e = np.arange(-p, n + p)
    if padding == "circular":
        return e % n
    if padding == "replicate":
        return np.clip(e, 0, n - 1)
    assert padding == "reflect" and p <= n - 1
    return np.where(e < 0, -e, np.where(e > n - 1, 2 * (n - 1) - e, e))


def conv64(x, k, padding, rate, phase, rule="legacy"):
    """A x in float64. x (B, C, H, W) float64 (may require grad), k (kv, kh). The padded image is gathered by index (so
    autograd scatters back through the boundary), then correlated with the flipped filter at stride `rate` from `phase`."""
    kv, kh = k.shape
    (sv, pv), (sh, ph) = axis_offsets(kv, rule), axis_offsets(kh, rule)
    B, C, H, W = x.shape
    iv = torch.from_numpy(pad_axis_index(H, pv, padding))
    ih = torch.from_numpy(pad_axis_index(W, ph, padding))
    xp = x[:, :, iv][:, :, :, ih]                                   # position e of the image <-> index e + p
    # y[i] = sum_a k[a] xp[i - a + s + p] = sum_t kf[t] xp[i + t + (s + p - (K-1))], kf the flipped filter
    ov, oh = sv + pv - (kv - 1), sh + ph - (kh - 1)
    assert ov >= 0 and oh >= 0
    xp = xp[:, :, ov + phase:, oh + phase:]
    y = F.conv2d(xp.reshape(B * C, 1, *xp.shape[-2:]), k.double().flip(0, 1)[None, None], stride=rate)
    ho, wo = (H - phase + rate - 1) // rate, (W - phase + rate - 1) // rate
    return y[:, :, :ho, :wo].reshape(B, C, ho, wo)


def reference64(x, k, padding, rate, phase, rule="legacy", ct=None):
    """(A x, A^T ct, ct) in float64: conv64 and its autograd (ct None: a random cotangent)."""
    x64 = x.detach().cpu().double().requires_grad_(True)
    y = conv64(x64, k.detach().cpu(), padding, rate, phase, rule)
    if ct is None:
        ct = torch.rand(y.shape, generator=torch.Generator().manual_seed(int(y.numel())))
    (gx,) = torch.autograd.grad(y, x64, ct.detach().cpu().double())
    return y.detach(), gx, ct


def axis_matrix64(n, taps, padding, rate, phase, rule="legacy"):
    """The (n_out, n) float64 matrix of one axis: the identity pushed through the same pad + strided conv along one axis (a
    1 x K filter on 1 x n rows)."""
    k = torch.as_tensor(np.asarray(taps, dtype=np.float64)).reshape(1, -1)
    eye = torch.eye(n, dtype=torch.float64).reshape(n, 1, 1, n)
    (sh, ph) = axis_offsets(k.shape[1], rule)
    ih = torch.from_numpy(pad_axis_index(n, ph, padding))
    xp = eye[:, :, :, ih][:, :, :, sh + ph - (k.shape[1] - 1) + phase:]
    y = F.conv2d(xp, k.flip(1)[None, None], stride=(1, rate))
    n_out = (n - phase + rate - 1) // rate
    return y[:, 0, 0, :n_out].T.contiguous().numpy()


def rand_kernel(kv, kh, seed):
    k = torch.rand((kv, kh), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return k / k.sum()
