"""Float64 restatement of the DRUNet denoiser and of the PlugAndPlay (DPIR half-quadratic splitting) baseline: the pinned
truth of tests/test_pnp_baseline.py and tests/test_pnp_baseline_gpu.py. Written from the published architecture (KAIR's
UNetRes, deepinv 0.2's DRUNet / get_DPIR_params / HQS / conjugate_gradient), independently of models/drunet.py and
models/pnp.py. Not collected."""
import math

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F


class ResBlockRef(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.res = nn.Sequential(nn.Conv2d(c, c, 3, padding=1, bias=False), nn.ReLU(), nn.Conv2d(c, c, 3, padding=1, bias=False))

    def forward(self, x):
        return x + self.res(x)


class DRUNetRef(nn.Module):
    """KAIR's UNetRes(in_nc=4, out_nc=3, act_mode 'R', strideconv / convtranspose, no bias) with its key names."""

    def __init__(self, nc=(64, 128, 256, 512), nb=4):
        super().__init__()
        self.m_head = nn.Conv2d(4, nc[0], 3, padding=1, bias=False)
        self.m_down1 = nn.Sequential(*[ResBlockRef(nc[0]) for _ in range(nb)], nn.Conv2d(nc[0], nc[1], 2, 2, bias=False))
        self.m_down2 = nn.Sequential(*[ResBlockRef(nc[1]) for _ in range(nb)], nn.Conv2d(nc[1], nc[2], 2, 2, bias=False))
        self.m_down3 = nn.Sequential(*[ResBlockRef(nc[2]) for _ in range(nb)], nn.Conv2d(nc[2], nc[3], 2, 2, bias=False))
        self.m_body = nn.Sequential(*[ResBlockRef(nc[3]) for _ in range(nb)])
        self.m_up3 = nn.Sequential(nn.ConvTranspose2d(nc[3], nc[2], 2, 2, bias=False), *[ResBlockRef(nc[2]) for _ in range(nb)])
        self.m_up2 = nn.Sequential(nn.ConvTranspose2d(nc[2], nc[1], 2, 2, bias=False), *[ResBlockRef(nc[1]) for _ in range(nb)])
        self.m_up1 = nn.Sequential(nn.ConvTranspose2d(nc[1], nc[0], 2, 2, bias=False), *[ResBlockRef(nc[0]) for _ in range(nb)])
        self.m_tail = nn.Conv2d(nc[0], 3, 3, padding=1, bias=False)

    def forward(self, x, sigma):
        x0 = torch.cat([x, torch.full_like(x[:, :1], sigma)], 1)
        x1 = self.m_head(x0)
        x2 = self.m_down1(x1)
        x3 = self.m_down2(x2)
        x4 = self.m_down3(x3)
        x = self.m_body(x4)
        x = self.m_up3(x + x4)
        x = self.m_up2(x + x3)
        x = self.m_up1(x + x2)
        return self.m_tail(x + x1)


def _q(t, on):
    """Through bfloat16 and back (round to nearest even) when `on`."""
    return t.to(torch.bfloat16).to(t.dtype) if on else t


def network_ref(sd, x, sigma, dtype, round_bf16=False, trace=None):
    """The network on an extent it runs directly, functionally from the state dict `sd`. With round_bf16, weights and
    every convolution input go through bfloat16; everything else stays in `dtype`. `trace` (a list) collects the max-abs of
    every activation."""
    nb = sum(1 for k in sd if k.startswith("m_body.") and k.endswith(".res.0.weight"))
    w = lambda key: _q(sd[key].to(dtype), round_bf16)          # noqa: E731

    def note(t):
        if trace is not None:
            trace.append(float(t.abs().max()))
        return t

    def conv(t, key, **kw):
        return note(F.conv2d(_q(t, round_bf16), w(key), **kw))

    def blocks(t, prefix, first):
        for i in range(first, first + nb):
            mid = note(torch.relu(conv(t, f"{prefix}.{i}.res.0.weight", padding=1)))
            t = note(t + conv(mid, f"{prefix}.{i}.res.2.weight", padding=1))
        return t

    x = x.to(dtype)
    x0 = torch.cat([x, torch.full_like(x[:, :1], sigma)], 1)
    skips = [conv(x0, "m_head.weight", padding=1)]
    t = skips[0]
    for lvl in (1, 2, 3):
        t = blocks(t, f"m_down{lvl}", 0)
        t = conv(t, f"m_down{lvl}.{nb}.weight", stride=2)
        skips.append(t)
    t = blocks(t, "m_body", 0)
    for lvl in (3, 2, 1):
        t = note(F.conv_transpose2d(_q(note(t + skips[lvl]), round_bf16), w(f"m_up{lvl}.0.weight"), stride=2))
        t = blocks(t, f"m_up{lvl}", 1)
    return conv(note(t + skips[0]), "m_tail.weight", padding=1)


def forward_ref(sd, x, sigma, dtype, round_bf16=False):
    """The eval-mode forward with its three extent paths (direct, replicate pad below 32, onesplit with refield 64)."""
    run = lambda v: network_ref(sd, v, sigma, dtype, round_bf16)      # noqa: E731
    x = x.to(dtype)
    h, w = x.shape[-2:]
    if h % 8 == 0 and w % 8 == 0 and h > 31 and w > 31:
        return run(x)
    if h < 32 or w < 32:
        ph, pw = int(math.ceil(h / 16) * 16 - h), int(math.ceil(w / 16) * 16 - w)
        return run(F.pad(x, (0, pw, 0, ph), mode="replicate"))[..., :h, :w]
    sh, sw = (h // 2 // 64 + 1) * 64, (w // 2 // 64 + 1) * 64
    if sh > h or sw > w:
        raise ValueError("a piece does not fit the image")
    tl, tr = run(x[..., :sh, :sw]), run(x[..., :sh, w - sw:])
    bl, br = run(x[..., h - sh:, :sw]), run(x[..., h - sh:, w - sw:])
    out = torch.zeros_like(x)
    out[..., :h // 2, :w // 2] = tl[..., :h // 2, :w // 2]
    out[..., :h // 2, w // 2:] = tr[..., :h // 2, sw - w + w // 2:]
    out[..., h // 2:, :w // 2] = bl[..., sh - h + h // 2:, :w // 2]
    out[..., h // 2:, w // 2:] = br[..., sh - h + h // 2:, sw - w + w // 2:]
    return out


def synthetic_state_dict(nc=(64, 128, 256, 512), nb=4, seed=0):
    """Random float32 weights with the real key set: the first convolution of a block at He scale (std sqrt(2 / fan_in)),
    the second at a quarter of the variance-preserving scale so that a block adds about 1/4 of its input's spread, the
    2x2 convolutions, the head and the tail variance-preserving (std sqrt(1 / fan_in))."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, p in DRUNetRef(nc, nb).state_dict().items():
        if p.shape[-1] == 2 and key.startswith("m_up"):
            fan_in = p.shape[0]                                  # ConvTranspose2d (Cin, Cout, 2, 2): one tap per output
        else:
            fan_in = p.shape[1] * p.shape[2] * p.shape[3]
        if key.endswith(".res.0.weight"):
            std = math.sqrt(2.0 / fan_in)
        elif key.endswith(".res.2.weight"):
            std = 0.25 * math.sqrt(1.0 / fan_in)
        else:
            std = math.sqrt(1.0 / fan_in)
        sd[key] = (torch.randn(p.shape, generator=g) * std).float()
    return sd


def assert_activation_range(sd, x, sigma, lo=1e-3, hi=1e3):
    """A condition on the fixture: the max-abs of every float64 activation of `x` lies in [lo, hi], so the relative bounds
    of the tests are neither met by vanishing signals nor strained by exploding ones."""
    trace = []
    network_ref(sd, x.double(), sigma, torch.float64, trace=trace)
    assert trace and lo <= min(trace) and max(trace) <= hi, (min(trace), max(trace))
    return min(trace), max(trace)


def dpir_params(s):
    sigma = np.logspace(np.log10(49.0 / 255.0), np.log10(s), 8).astype(np.float32)
    step = (sigma / max(0.01, s)) ** 2 / 0.23
    return [float(v) for v in sigma], [float(v) for v in step]


def cg_ref(op, b, max_iter, tol):
    x = torch.zeros_like(b)
    r = b.clone()
    p = r
    rs = (r * r).sum()
    for _ in range(max_iter):
        Ap = op(p)
        alpha = rs / (p * Ap).sum()
        x = x + alpha * p
        r = r - alpha * Ap
        rs_new = (r * r).sum()
        if math.sqrt(float(rs_new)) < tol:
            break
        p = r + (rs_new / rs) * p
        rs = rs_new
    return x


def pnp_ref(y, A, At, sd, noise_level_img, dtype, round_bf16=False, early_stop=False, cg_max_iter=50, cg_tol=1e-3):
    """HQS with the DPIR schedule in `dtype`; A / At are callables in that dtype. Returns (x, iterations run)."""
    s = 1e-5 if noise_level_img == 0 else noise_level_img
    sigmas, steps = dpir_params(s)
    y = y.to(dtype)
    x = At(y)
    ran = 0
    for k in range(8):
        x_prev = x
        gamma = steps[k]
        u = cg_ref(lambda v: At(A(v)) + v / gamma, At(y) + x / gamma, cg_max_iter, cg_tol)
        x = forward_ref(sd, u, sigmas[k], dtype, round_bf16)
        ran = k + 1
        if early_stop and k > 1:
            if float(torch.linalg.vector_norm(x_prev - x) / (torch.linalg.vector_norm(x) + 1e-6)) < 1e-5:
                break
    return x, ran
