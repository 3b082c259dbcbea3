"""The BM3D deblurring baseline (reference: src/models/bm3d_deblurring.py, which calls `bm3d.bm3d_deblurring(z, sigma, psf)`
on one channel of one image at a time in numpy). The bm3d package is not part of the reference tree, so the algorithm is
restated here from the published method (Dabov, Foi, Katkovnik, Egiazarian: BM3D 2007, BM3D-DEB 2008) and from recollection
of the package's structure; parity with the package is UNPINNED. The pinned truth is the float64 restatement
tests/bm3d_ref.py.

One plane is z of extent H x W (every channel of every image is a plane of its own, as in the reference). V is the
unnormalised fft2 of the blur kernel zero-padded to H x W with its centre rolled to the origin (`otf`), s2 = sigma_psd^2 =
(noise_level / 255)^2, n = H W. Four steps:

1. Regularised inverse. G1 = conj(V) / (|V|^2 + 4e-4 s2 n); z1 = real(ifft2(fft2(z) G1)); noise spectrum S1 = s2 |G1|^2.
2. Hard-thresholding stage on z1 with spectrum S1: the pilot p.
3. Regularised Wiener inverse. P2 = |fft2(p)|^2; G2 = conj(V) P2 / (P2 |V|^2 + 5e-3 s2 n); z2 = real(ifft2(fft2(z) G2));
   S2 = s2 |G2|^2.
4. Wiener stage on z2 with pilot p and spectrum S2: the result.

A stage:
- Blocks are 8 x 8 and never wrap. The reference positions of an axis of extent m are 0, step, 2 step ... up to m - 8, and
  m - 8 itself if that sequence misses it; step = 3.
- Matching (on z1 in step 2, on the pilot in step 4; sei_bm3d_match). The candidates of the reference block at (r, c) are all
  block positions (r', c') inside the image with |r' - r| <= 19 and |c' - c| <= 19; d = sum(diff^2) / 64. Keep those with
  d <= tau, sorted ascending by (d, r', c'), take the first n_max and cut to the largest power of two not above their number.
  tau = 3000 / 255^2 and n_max = 16 for hard thresholding, 400 / 255^2 and 32 for Wiener (the `np` profile on the [0, 1] scale).
- 3-D transform: the orthonormal 8 x 8 DCT-II of every block, then the full orthonormal Haar decomposition along the group
  (pairs (a + b) / sqrt 2 and (a - b) / sqrt 2, recursing on the sums).
- Coefficient variances (`coefficient_variances`): for the 2-D DCT coefficient i = (p, q), v_i = (1 / n) sum_xi S(xi)
  |Psi_i(xi)|^2 with Psi_i the fft2 of the basis function zero-padded to H x W; the basis is separable, so this is an
  (8 x H)(H x W)(W x 8) product per plane. Every group coefficient (k, i) is given the variance v_i.
- Hard thresholding (sei_bm3d_ht): keep a coefficient when |c| > 2.7 sqrt(v_i); group weight w = 1 / (sum of v_i over the
  kept coefficients), 1 when none is kept.
- Wiener (sei_bm3d_wiener): the group is taken at the same positions from the noisy plane and from the pilot; shrinkage
  W = P^2 / (P^2 + v_i) on the pilot's coefficients P; w = 1 / sum(W^2 v_i) over all coefficients of the group (1 when the
  sum is 0).
- Aggregation: invert both transforms; num += w K block, den += w K with K = outer(kaiser(8, 2.0), kaiser(8, 2.0)); the
  output is num / den (sei_bm3d_finish). Every pixel is covered: the last position of each axis is a reference position.

Deliberate deviations from the package:
- The 2-D transform is the DCT in both stages (the package uses bior1.5 in the first).
- Variances are per 2-D coefficient and the blocks of a group are treated as independent: the 2008 BM3D-DEB scheme, not the
  package's exact per-group variances.
- No refiltering and no profile argument.
- sigma_psd is a scalar, which is all the reference ever passes.
- sigma_psd <= 0 raises ValueError: both inversions divide by terms proportional to it.

The two inversions and the variances are plumbing (torch.fft and torch matmuls on the device, as noise2inverse.py, in float64:
`regularised_inverse` says why); matching
and the two collaborative filters are the HIP kernels of csrc/bm3d_kernels.hip, all planes of the batch per launch. The
aggregation adds with float atomics: a stage's output is reproducible to rounding, not to the bit; matching is bit-exact.
"""
import numpy as np
import torch
from torch.nn import Module

import _native as N

TAU_HT, TAU_WIENER = 3000 / 255 ** 2, 400 / 255 ** 2
N_MAX_HT, N_MAX_WIENER = 16, 32
LAMBDA_3D = 2.7
REG_INVERSE, REG_WIENER = 4e-4, 5e-3
STEP, WINDOW = 3, 39
_N_MAX = (1, 2, 4, 8, 16, 32)


def _staged(t):
    """`t` as the kernels need it: contiguous and on the 4-byte grid (a copy only where it is not)."""
    t = t.contiguous()
    return t if N.aligned(t, to=4) else t.clone()


def _planes(t, name):
    N.check_tensor(t.contiguous() if isinstance(t, torch.Tensor) else t, name)
    if t.dim() < 2 or t.shape[-2] < 8 or t.shape[-1] < 8:
        raise ValueError(f"{name}: expected (..., H, W) with H, W >= 8 (blocks are 8 x 8), got {tuple(t.shape)}")
    t = _staged(t.detach())
    H, W = t.shape[-2:]
    return t, t.numel() // (H * W), H, W


def otf(kernel, H, W, legacy=False, dtype=torch.float32):
    """V: the unnormalised fft2 of `kernel` (.., kh, kw) zero-padded to H x W with its centre (kh // 2, kw // 2) rolled to
    the origin, as BlurV2.A convolves (taps that do not fit wrap around). legacy: the circular `Blur`, which reads an axis
    with an even number of taps one position further back: a zero tap in front of such an axis first. Complex of the
    precision of `dtype`."""
    k = kernel.detach().reshape(kernel.shape[-2], kernel.shape[-1]).to(dtype)
    if legacy:
        k = torch.nn.functional.pad(k, (1 - k.shape[1] % 2, 0, 1 - k.shape[0] % 2, 0))
    kh, kw = k.shape
    rows = (torch.arange(kh, device=k.device) - kh // 2) % H
    cols = (torch.arange(kw, device=k.device) - kw // 2) % W
    psf = torch.zeros((H, W), dtype=dtype, device=k.device)
    psf.index_put_((rows[:, None].expand(kh, kw), cols[None, :].expand(kh, kw)), k, accumulate=True)
    return torch.fft.fft2(psf)


def _basis_power(m, device, dtype):
    """(8, m): |fft(d_p zero-padded to m)|^2 for the eight DCT basis vectors d_p."""
    j, i = np.arange(8)[:, None], np.arange(8)[None, :]
    D = np.sqrt(2.0 / 8) * np.cos(np.pi * (2 * i + 1) * j / 16)
    D[0] /= np.sqrt(2.0)
    return (torch.fft.fft(torch.from_numpy(D), n=m, dim=1).abs() ** 2).to(device=device, dtype=dtype)


def coefficient_variances(S):
    """(planes, H, W) noise spectra -> (planes, 64) variances of the 8 x 8 DCT coefficients, index p * 8 + q with p the
    vertical frequency, in the precision of S."""
    if S.dim() != 3:
        raise ValueError(f"coefficient_variances: expected (planes, H, W), got {tuple(S.shape)}")
    H, W = S.shape[-2:]
    A, B = _basis_power(H, S.device, S.dtype), _basis_power(W, S.device, S.dtype)
    v = torch.matmul(torch.matmul(A, S), B.t()) / float(H * W)
    return v.reshape(S.shape[0], 64).contiguous()


def ref_blocks(H, W, step=STEP):
    n = N.lib().sei_bm3d_ref_blocks(int(H), int(W), int(step))
    if n == 0:
        raise N.NativeLibraryError(f"sei_bm3d_ref_blocks refuses {H} x {W} at step {step}")
    return n


def bm3d_match(img, tau, n_max, step=STEP, window=WINDOW, return_distances=False):
    """Groups of every plane of `img` (..., H, W): (positions, counts), int32 of shapes (planes, refs, n_max, 2) and
    (planes, refs); with return_distances also the kept distances (planes, refs, n_max), +inf behind the count."""
    img, planes, H, W = _planes(img, "img")
    n_max, step, window = int(n_max), int(step), int(window)
    if n_max not in _N_MAX or step < 1 or window < 1 or window % 2 == 0 or not tau >= 0:
        raise ValueError(f"bm3d_match: n_max in {_N_MAX}, step >= 1, an odd window and tau >= 0, got {n_max}, {step}, "
                         f"{window}, {tau}")
    refs = ref_blocks(H, W, step)
    pos = torch.empty((planes, refs, n_max, 2), dtype=torch.int32, device=img.device)
    counts = torch.empty((planes, refs), dtype=torch.int32, device=img.device)
    dist = torch.empty((planes, refs, n_max), dtype=torch.float32, device=img.device) if return_distances else None
    N.call("sei_bm3d_match", img.data_ptr(), planes, H, W, step, window, float(tau), n_max, pos.data_ptr(),
           counts.data_ptr(), N.ptr(dist))
    return (pos, counts, dist) if return_distances else (pos, counts)


def _checked_groups(groups, planes, H, W, step, who):
    """Injected groups, validated on the host before anything is launched (one synchronisation, on this path only)."""
    pos, counts = groups
    N.check_tensor(pos, f"{who}: positions", dtype=torch.int32)
    N.check_tensor(counts, f"{who}: counts", dtype=torch.int32)
    refs = ref_blocks(H, W, step)
    if pos.dim() != 4 or tuple(pos.shape[:2]) != (planes, refs) or pos.shape[2] not in _N_MAX or pos.shape[3] != 2 or \
            tuple(counts.shape) != (planes, refs):
        raise ValueError(f"{who}: groups of shapes {tuple(pos.shape)}, {tuple(counts.shape)} for {planes} planes of "
                         f"{refs} reference blocks")
    n_max = pos.shape[2]
    rows, cols = pos[..., 0], pos[..., 1]
    ok = (rows >= 0) & (rows <= H - 8) & (cols >= 0) & (cols <= W - 8)
    good = (counts >= 1) & (counts <= n_max) & ((counts & (counts - 1)) == 0)
    if not (bool(ok.all()) and bool(good.all())):
        raise ValueError(f"{who}: group positions outside [0, {H - 8}] x [0, {W - 8}] or counts that are no power of two "
                         f"in [1, {n_max}]")
    return pos, counts, n_max


def _variances(variances, planes, who):
    N.check_tensor(variances.contiguous() if isinstance(variances, torch.Tensor) else variances, f"{who}: variances")
    if tuple(variances.shape) != (planes, 64):
        raise ValueError(f"{who}: variances of shape {tuple(variances.shape)} for {planes} planes")
    return _staged(variances.detach())


def _finish(work, like, planes, H, W):
    out = torch.empty_like(like)
    N.call("sei_bm3d_finish", work.data_ptr(), out.data_ptr(), planes, H, W)
    return out


def bm3d_ht(noisy, variances, groups=None, lambd=LAMBDA_3D, tau=TAU_HT, n_max=N_MAX_HT, step=STEP, window=WINDOW, agg=0,
            return_coefficients=False):
    """The hard-thresholding stage on every plane of `noisy` (..., H, W) with variances (planes, 64). groups = None matches
    on `noisy` (tau, n_max); given groups (positions, counts) are validated on the host first. agg: 0 sums a tile's blocks
    in LDS before the global atomics, 1 adds every block to global memory. With return_coefficients also the transform
    coefficients before the shrinkage, float64 (planes, refs, n_max, 64), zero behind a group's count."""
    noisy, planes, H, W = _planes(noisy, "noisy")
    var = _variances(variances, planes, "bm3d_ht")
    if not lambd >= 0:
        raise ValueError(f"bm3d_ht: lambd must not be negative, got {lambd}")
    if groups is None:
        pos, counts = bm3d_match(noisy, tau, n_max, step, window)
    else:
        pos, counts, n_max = _checked_groups(groups, planes, H, W, step, "bm3d_ht")
    work = torch.empty((2,) + tuple(noisy.shape), dtype=torch.float32, device=noisy.device)
    coef = torch.zeros(tuple(pos.shape[:3]) + (64,), dtype=torch.float64, device=noisy.device) if return_coefficients \
        else None
    N.call("sei_bm3d_ht", noisy.data_ptr(), var.data_ptr(), pos.data_ptr(), counts.data_ptr(), planes, H, W, int(step),
           int(n_max), int(window), float(lambd), int(agg), work.data_ptr(), N.ptr(coef))
    out = _finish(work, noisy, planes, H, W)
    return (out, coef) if return_coefficients else out


def bm3d_wiener(noisy, pilot, variances, groups=None, tau=TAU_WIENER, n_max=N_MAX_WIENER, step=STEP, window=WINDOW, agg=0):
    """The Wiener stage on every plane of `noisy` with the pilot of the same shape. groups = None matches on `pilot`."""
    noisy, planes, H, W = _planes(noisy, "noisy")
    pilot, planes_p, Hp, Wp = _planes(pilot, "pilot")
    if (planes_p, Hp, Wp) != (planes, H, W):
        raise ValueError(f"bm3d_wiener: pilot of shape {tuple(pilot.shape)} for noisy planes of shape {tuple(noisy.shape)}")
    var = _variances(variances, planes, "bm3d_wiener")
    if groups is None:
        pos, counts = bm3d_match(pilot, tau, n_max, step, window)
    else:
        pos, counts, n_max = _checked_groups(groups, planes, H, W, step, "bm3d_wiener")
    work = torch.empty((2,) + tuple(noisy.shape), dtype=torch.float32, device=noisy.device)
    N.call("sei_bm3d_wiener", noisy.data_ptr(), pilot.data_ptr(), var.data_ptr(), pos.data_ptr(), counts.data_ptr(), planes,
           H, W, int(step), int(n_max), int(window), int(agg), work.data_ptr())
    return _finish(work, noisy, planes, H, W)


def _power(c):
    return c.real ** 2 + c.imag ** 2


def regularised_inverse(z, V, sigma_psd, pilot=None):
    """Step 1 (pilot None) or step 3 on planes z (planes, H, W) with the transfer function V (H, W): the inverse-filtered
    planes and the (planes, 64) coefficient variances of their noise, both float32. The arithmetic is float64 on the device:
    the inverse has a gain of up to 1 / (2 sqrt(reg s2 n)), about 30 at 5 / 255, which carries a float32 FFT's rounding to a
    few 1e-6 of the planes, enough to flip matching and thresholding decisions of the stage that follows; three planes of
    256 x 384 cost microseconds either way."""
    H, W = z.shape[-2:]
    s2, n = float(sigma_psd) ** 2, H * W
    z, V = z.to(torch.float64), V.to(torch.complex128)
    V2 = _power(V)
    if pilot is None:
        G = (V.conj() / (V2 + REG_INVERSE * s2 * n)).expand(z.shape[0], H, W)
    else:
        P2 = _power(torch.fft.fft2(pilot.to(torch.float64)))
        G = V.conj() * P2 / (P2 * V2 + REG_WIENER * s2 * n)
    out = torch.fft.ifft2(torch.fft.fft2(z) * G).real
    return out.to(torch.float32).contiguous(), coefficient_variances(s2 * _power(G)).to(torch.float32)


class BM3D(Module):
    """The reference's BM3D(physics, sigma_psd): the blur kernel is physics.kernel, or physics.filter for the legacy Blur.
    No parameters: its state dict is empty."""

    def __init__(self, physics, sigma_psd):
        super().__init__()
        kernel, legacy = getattr(physics, "kernel", None), False
        if kernel is None:
            kernel, legacy = getattr(physics, "filter", None), True
        if kernel is None:
            raise NotImplementedError("model kind 'BM3D' deconvolves with the physics' blur kernel: a folder of measurements "
                                      "without a physics, or a task without a blur kernel, stays outside what this build "
                                      "can run")
        sigma_psd = float(sigma_psd)
        if not sigma_psd > 0:
            raise ValueError(f"BM3D: sigma_psd must be positive (both inversions divide by terms proportional to it), got "
                             f"{sigma_psd}")
        self.sigma_psd = sigma_psd
        self.kernel = kernel.detach()
        self.legacy = legacy

    @torch.no_grad()
    def forward(self, y):
        N.check_tensor(y.contiguous() if isinstance(y, torch.Tensor) else y, "y")
        if y.dim() < 2:
            raise ValueError("BM3D: expected an image tensor (..., H, W)")
        H, W = y.shape[-2:]
        z = y.contiguous().reshape(-1, H, W)
        V = otf(self.kernel.to(y.device), H, W, self.legacy, dtype=torch.float64)
        z1, v1 = regularised_inverse(z, V, self.sigma_psd)
        p = bm3d_ht(z1, v1)
        z2, v2 = regularised_inverse(z, V, self.sigma_psd, pilot=p)
        return bm3d_wiener(z2, p, v2).reshape(y.shape)
