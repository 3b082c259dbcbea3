"""Evaluation metrics of the path: PSNR and SSIM on the luma channel (reference: src/metrics.py).

Both restate kornia.color.rgb_to_ycbcr's Y (0.299 R + 0.587 G + 0.114 B) and torchmetrics' definitions with data_range 1.
kornia and torchmetrics are absent here, so the restatements are pinned only against the oracle's own (PSNR:
oracle/torch_path.py: psnr_y) or against a float64 restatement in the tests (SSIM) -- SURVEY 8c "parity unpinned" for
this row.

- `psnr_fn`: torchmetrics.functional.peak_signal_noise_ratio = 10 log10(1 / mse). On GPU tensors the squared-error sum
  runs in sei_luma_sqerr.
- `ssim_fn`: torchmetrics.functional.structural_similarity_index_measure with its defaults: an 11-tap Gaussian window of
  sigma 1.5 per axis (exp(-(i / 1.5)^2 / 2), i = -5..5, normalised), the five weighted moments mu_x, mu_y, E[x^2], E[y^2],
  E[xy] per window, sigma_x^2 = max(E[x^2] - mu_x^2, 0) and sigma_y^2 likewise (current torchmetrics clamps both at 0),
  sigma_xy = E[xy] - mu_x mu_y, C1 = 0.01^2, C2 = 0.03^2, and
  ssim = (2 mu_x mu_y + C1)(2 sigma_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(sigma_x^2 + sigma_y^2 + C2)).
  torchmetrics reflect-pads by 5 and then crops 5 from every side of the map: the two cancel, so only the windows that
  lie inside the image count ((H-10) x (W-10) of them, H, W >= 11), and the result is the mean of that map per image.
  Unpinned beyond that restatement: the torchmetrics version the reference ran (its clamp, its float32 window taps).
  On float32 GPU tensors it runs in sei_ssim_luma; on CPU tensors as separable conv2d in the input dtype. Both compute
  the moments of the luma minus a local constant (per tile on the GPU, per image on the host): the variances and the
  covariance do not change, and the float32 cancellation of E[x^2] - mu^2 no longer scales with the image's level.
- LPIPS (pyiqa, pretrained AlexNet weights) is not rebuilt: `compute_metrics` returns NaN for it.
"""
import math

import torch
import torch.nn.functional as F

SSIM_TAPS = 11
_C1, _C2 = 0.01 ** 2, 0.03 ** 2


def luma(img):
    r, g, b = img[..., 0, :, :], img[..., 1, :, :], img[..., 2, :, :]
    return 0.299 * r + 0.587 * g + 0.114 * b


def psnr_fn(x_hat, x):
    """x_hat, x: (3, H, W) in [0, 1] -> scalar tensor (dB)."""
    if x_hat.is_cuda and x.is_cuda and x_hat.dtype == torch.float32 and x.dtype == torch.float32:
        import _native as N
        a, b = x_hat.contiguous(), x.contiguous()
        npix = a.shape[-2] * a.shape[-1]
        out = torch.empty(1, dtype=torch.float32, device=a.device)
        work = torch.empty(256, dtype=torch.float32, device=a.device)
        N.call("sei_luma_sqerr", a.data_ptr(), b.data_ptr(), npix, out.data_ptr(), work.data_ptr())
        err = out[0] / npix
    else:
        err = (luma(x_hat) - luma(x)).pow(2).mean()
    return 10.0 * torch.log10(1.0 / err)


def gaussian_taps(dtype=torch.float64, device="cpu"):
    """torchmetrics' _gaussian(11, 1.5), computed in float64 and rounded to `dtype`."""
    d = torch.arange(-(SSIM_TAPS // 2), SSIM_TAPS // 2 + 1, dtype=torch.float64)
    g = torch.exp(-((d / 1.5) ** 2) / 2)
    return (g / g.sum()).to(dtype=dtype, device=device)


def _ssim_host(a, b):
    """(B, 3, H, W) pairs -> (B,) in the input dtype: separable conv2d over the stacked moments."""
    ya, yb = luma(a), luma(b)                                   # (B, H, W)
    ca = ya.mean(dim=(-2, -1), keepdim=True)
    cb = yb.mean(dim=(-2, -1), keepdim=True)
    ya, yb = ya - ca, yb - cb
    B, H, W = ya.shape
    g = gaussian_taps(ya.dtype, ya.device)
    stack = torch.stack((ya, yb, ya * ya, yb * yb, ya * yb), dim=1).reshape(B * 5, 1, H, W)
    m = F.conv2d(F.conv2d(stack, g.view(1, 1, 1, -1)), g.view(1, 1, -1, 1)).reshape(B, 5, H - 10, W - 10)
    mu_a, mu_b, e_aa, e_bb, e_ab = m.unbind(1)
    var_a = (e_aa - mu_a * mu_a).clamp(min=0)
    var_b = (e_bb - mu_b * mu_b).clamp(min=0)
    cov = e_ab - mu_a * mu_b
    mu_a, mu_b = mu_a + ca, mu_b + cb
    ssim_map = (2 * mu_a * mu_b + _C1) * (2 * cov + _C2) / ((mu_a * mu_a + mu_b * mu_b + _C1) * (var_a + var_b + _C2))
    return ssim_map.mean(dim=(-2, -1))


def ssim_fn(x_hat, x):
    """x_hat, x: (3, H, W) in [0, 1] -> scalar tensor, or (B, 3, H, W) -> (B,); symmetric in its arguments.
    Float32 GPU tensors run sei_ssim_luma (no other GPU dtype: there is no eager fallback); CPU tensors the host path."""
    if x_hat.shape != x.shape:
        raise ValueError(f"ssim_fn: shapes differ: {tuple(x_hat.shape)} vs {tuple(x.shape)}")
    if x.dim() not in (3, 4) or x.shape[-3] != 3:
        raise ValueError(f"ssim_fn: expected (3, H, W) or (B, 3, H, W) RGB images, got {tuple(x.shape)}")
    H, W = x.shape[-2:]
    if H < SSIM_TAPS or W < SSIM_TAPS:
        raise ValueError(f"ssim_fn: images must be at least {SSIM_TAPS} x {SSIM_TAPS} (the Gaussian window), got {H} x {W}")
    if x_hat.device != x.device:
        raise ValueError(f"ssim_fn: operands on {x_hat.device} and {x.device}")
    batched = x.dim() == 4
    a, b = (x_hat, x) if batched else (x_hat[None], x[None])
    if not x.is_cuda:
        out = _ssim_host(a, b)
        return out if batched else out[0]
    import _native as N
    if x_hat.dtype != torch.float32 or x.dtype != torch.float32:
        raise TypeError(f"ssim_fn: GPU operands must be float32, got {x_hat.dtype} and {x.dtype}")
    a, b = a.contiguous(), b.contiguous()       # (4-byte alignment is all the kernel needs: offset views pass as they are)
    n = a.shape[0]
    out = torch.empty(n, dtype=torch.float32, device=a.device)
    work = torch.empty(N.lib().sei_ssim_luma_work_floats(n, H, W), dtype=torch.float32, device=a.device)
    N.call("sei_ssim_luma", a.data_ptr(), b.data_ptr(), n, H, W, out.data_ptr(), work.data_ptr())
    return out if batched else out[0]


def register_fn(x, x_hat):
    """Centre-crop both images to their common size (reference :33-40, torchvision CenterCrop)."""
    if x.shape[-2] != x_hat.shape[-2] or x.shape[-1] != x_hat.shape[-1]:
        hmin, wmin = min(x.shape[-2], x_hat.shape[-2]), min(x.shape[-1], x_hat.shape[-1])

        def centre(t):
            top = int(round((t.shape[-2] - hmin) / 2.0))
            left = int(round((t.shape[-1] - wmin) / 2.0))
            return t[..., top:top + hmin, left:left + wmin]
        x, x_hat = centre(x), centre(x_hat)
    return x, x_hat


def compute_metrics(x, x_hat, ssim=False):
    """(psnr, ssim, lpips) as the reference's compute_metrics. The SSIM is computed with ssim=True (test.py --ssim) and
    NaN otherwise; the LPIPS is always NaN."""
    x, x_hat = register_fn(x, x_hat)
    ssim_val = ssim_fn(x, x_hat).item() if ssim else math.nan
    return psnr_fn(x, x_hat).item(), ssim_val, math.nan
