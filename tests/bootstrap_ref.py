"""CPU reference of the equivariant bootstrap (bootstrap.py, the sei_boot_* kernels): plain torch, float64 unless a dtype
is named, and nothing of the library under test is imported. tests/test_bootstrap.py anchors it to F.grid_sample on the
reference-order grid and measures its pull-back's interpolation error; tests/test_bootstrap_gpu.py holds the kernels to it.

The one step that is defined in float32 is the quantisation q(t) = clamp(round(t * 255) / 255, 0, 1) of test.py: its input is
a float32 image, a tie of the float32 product rounds to even, and the division is the correctly rounded float32 one. `quantize`
therefore runs torch's float32 chain on the CPU on the float32 rounding of its input, whatever precision surrounds it.
"""
import math

import torch
import torch.nn.functional as F

LUMA = (0.299, 0.587, 0.114)


def base_grid(H, W, dtype=torch.float64):
    """(H, W, 2) normalised (x, y) of pixel (i, j): x = (2 / W) j - 1 from the column, y = (2 / H) i - 1 from the row."""
    x = 2 / W * torch.arange(W, dtype=dtype) - 1
    y = 2 / H * torch.arange(H, dtype=dtype) - 1
    return torch.stack([x[None, :].expand(H, W), y[:, None].expand(H, W)], dim=-1)


def forward_grid(H, W, rate, center, dtype=torch.float64):
    """(B, H, W, 2): (g - c) / rate + c, in the operation order of the float32 chain (1 / rate first)."""
    B = rate.numel()
    g, c = base_grid(H, W, dtype)[None], center.to(dtype).reshape(B, 1, 1, 2)
    return 1 / rate.to(dtype).reshape(B, 1, 1, 1) * (g - c) + c


def pullback_grid(H, W, rate, center, dtype=torch.float64):
    """(B, H, W, 2): rate (g - c) + c."""
    B = rate.numel()
    g, c = base_grid(H, W, dtype)[None], center.to(dtype).reshape(B, 1, 1, 2)
    return rate.to(dtype).reshape(B, 1, 1, 1) * (g - c) + c


def sample(x, grid):
    return F.grid_sample(x, grid, mode="bicubic", padding_mode="reflection", align_corners=True)


def zoom_out(x, rate, center, dtype=torch.float64):
    """a_r = T_r x for one (C, H, W) image and B replicas -> (B, C, H, W)."""
    C, H, W = x.shape
    B = rate.numel()
    return sample(x.to(dtype)[None].expand(B, C, H, W), forward_grid(H, W, rate, center, dtype))


def pull_back(d, rate, center, dtype=torch.float64):
    """T_r^+ d_r for (B, H, W) planes -> (B, H, W)."""
    B, H, W = d.shape
    return sample(d.to(dtype)[:, None], pullback_grid(H, W, rate, center, dtype))[:, 0]


def quantize(t):
    """test.py's quantize_and_clamp as torch's float32 chain on the CPU; the result in the dtype of `t`."""
    t32 = t.to(torch.float32)
    return ((t32 * 255.0).round() / 255.0).clamp(0.0, 1.0).to(t.dtype)


def luma(img):
    r, g, b = img[..., 0, :, :], img[..., 1, :, :], img[..., 2, :, :]
    return LUMA[0] * r + LUMA[1] * g + LUMA[2] * b


def luma_diff(a, b, dtype=torch.float64):
    """d = Y(q(a)) - Y(q(b)) for (..., 3, H, W) images, in `dtype` (float32: torch's chain, the kernel's bits)."""
    return luma(quantize(a.to(dtype))) - luma(quantize(b.to(dtype)))


def circular_blur(x, kernel):
    """y[i, j] = sum_{a, b} k[a, b] x[(i - a + kv // 2) mod H, (j - b + kh // 2) mod W] per plane (BlurV2.A)."""
    kv, kh = kernel.shape
    y = torch.zeros_like(x)
    for a in range(kv):
        for b in range(kh):
            y = y + kernel[a, b].to(x.dtype) * torch.roll(x, shifts=(a - kv // 2, b - kh // 2), dims=(-2, -1))
    return y


def psnr(m):
    return 10.0 * math.log10(1.0 / m) if m > 0 else math.inf


def summarise(mse):
    """(EST_PSNR, EST_PSNR_Q90) of the (N,) mean squared errors."""
    host = sorted(float(v) for v in mse.double())
    n = len(host)
    return psnr(sum(host) / n), psnr(host[math.ceil(0.9 * n) - 1])


def bootstrap(x_hat, rate, center, noise, A, sigma, model=lambda v: v, dtype=torch.float64):
    """The whole estimate for one (3, H, W) reconstruction with the draws given: rate (N,), center (N, 2), unit normal
    noise of the shape of A(a). A and model are callables on (N, C, h, w) tensors of `dtype`.
    -> dict: a, b (N, 3, H, W), d (N, H, W), mse (N,), msq, rmse (H, W), est_psnr, est_psnr_q90."""
    n = rate.numel()
    a = zoom_out(x_hat, rate, center, dtype)
    b = model(A(a) + sigma * noise.to(dtype))
    d = luma_diff(a, b, dtype)
    H, W = d.shape[-2:]
    mse = (d * d).sum(dim=(-2, -1)) / (H * W)
    back = pull_back(d, rate, center, dtype)
    msq = (back * back).sum(0)
    out = {"a": a, "b": b, "d": d, "mse": mse, "msq": msq, "rmse": (msq / n).sqrt()}
    out["est_psnr"], out["est_psnr_q90"] = summarise(mse)
    return out
