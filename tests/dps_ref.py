"""Restatement of deepinv 0.2's sampling.DPS (as recalled: tables, schedule, forward) around any callable denoiser with
autograd, in any dtype, and what the tests of the DRUNet's vector-Jacobian product need: the network of drunet_ref with its
ReLUs replaced by given masks, the pre-activation signs of the plain forward, and the transposed network written out by
hand (so that the bf16 roundings of the backward pass can be placed where the kernels place them). The pinned truth of
tests/test_dps_baseline.py and tests/test_dps_baseline_gpu.py; written with torch tensors and the state dict's own weights,
independently of models/dps.py (numpy tables) and models/drunet.py (packed transposed weights). Not collected."""
import math

import numpy as np
import torch
from torch.nn import functional as F

from drunet_ref import _q

T = 1000


def tables_ref():
    """(betas, ac): float32 torch tensors of length 1000 and 1001; alpha(t) = ac[t + 1]."""
    betas = torch.from_numpy(np.linspace(1e-4, 2e-2, T, dtype=np.float32))
    return betas, torch.cumprod(1.0 - torch.cat([torch.zeros(1), betas]), dim=0)


def schedule_ref(max_iter):
    skip = T // max_iter
    seq = range(0, T, skip)
    seq_next = [-1] + list(seq[:-1])
    return list(zip(reversed(seq), reversed(seq_next)))


def coefficients_ref(at, an, eta=1.0):
    """(sigma of the denoiser, st, c2) of a step, in float64."""
    st = eta * math.sqrt((1 - at / an) * (1 - an) / (1 - at))
    return math.sqrt(1 - at) / math.sqrt(at) / 2, st, math.sqrt(max((1 - an) - st ** 2, 0.0))


def dps_step_ref(x, y, A, D, nz, at, an, eta=1.0, stats=None):
    """One sampling step in x's dtype. D(aux, sigma) must be differentiable by autograd; A a callable in that dtype.
    `stats` (a dict) collects every f_b, the least distance of |2 out - 1| from 1 and the clamped / total pixel counts."""
    sigma, st, c2 = coefficients_ref(at, an, eta)
    with torch.enable_grad():
        xg = x.detach().requires_grad_(True)
        out = D(xg / (2 * math.sqrt(at)) + 0.5, sigma)
        t = 2 * out - 1
        x0 = t.clamp(-1, 1)
        r = A(x0 / 2 + 0.5) - y
        f = 0.5 * (r * r).flatten(1).sum(1)
        pos = f > 0                                              # sqrt has no derivative at 0: such an image gets g = 0
        g = torch.autograd.grad(torch.sqrt(f[pos]).sum(), xg)[0] if bool(pos.any()) else torch.zeros_like(x)
    x0, t = x0.detach(), t.detach()
    if stats is not None:
        stats.setdefault("f", []).extend(float(v) for v in f.detach())
        stats["edge"] = min(stats.get("edge", math.inf), float((t.abs() - 1).abs().min()))
        stats["clamped"] = stats.get("clamped", 0) + int((t.abs() > 1).sum())
        stats["pixels"] = stats.get("pixels", 0) + t.numel()
    return (math.sqrt(an) - c2 * math.sqrt(at) / math.sqrt(1 - at)) * x0 + st * nz + c2 * x / math.sqrt(1 - at) - g


def dps_ref(y, A, D, draws, max_iter, dtype, eta=1.0, stats=None):
    """DPS.forward in `dtype` with the float32 table: draws[0] is the start (the image's shape), draws[k + 1] the noise of
    step k."""
    _, ac = tables_ref()
    y = y.to(dtype)
    x = draws[0].to(dtype)
    for k, (i, j) in enumerate(schedule_ref(max_iter)):
        x = dps_step_ref(x, y, A, D, draws[k + 1].to(dtype), float(ac[i + 1]), float(ac[j + 1]), eta, stats)
    return x / 2 + 0.5


# ---- the DRUNet with its ReLUs fixed ----

def _nb(sd):
    return sum(1 for k in sd if k.startswith("m_body.") and k.endswith(".res.0.weight"))


def masked_network_ref(sd, x, sigma, masks, dtype, round_bf16=False, signs=None):
    """drunet_ref.network_ref with relu(v) replaced by v * masks[k] for the k-th ResBlock in network order (m_down1 ..
    m_down3, m_body, m_up3 .. m_up1). With masks None the ReLUs stay, and `signs` (a list) collects [v > 0]."""
    nb = _nb(sd)
    w = lambda key: _q(sd[key].to(dtype), round_bf16)          # noqa: E731
    conv = lambda t, key, **kw: F.conv2d(_q(t, round_bf16), w(key), **kw)      # noqa: E731
    it = iter(masks) if masks is not None else None

    def blocks(t, prefix, first):
        for i in range(first, first + nb):
            pre = conv(t, f"{prefix}.{i}.res.0.weight", padding=1)
            if it is None:
                if signs is not None:
                    signs.append(pre.detach() > 0)
                mid = torch.relu(pre)
            else:
                mid = pre * next(it).to(dtype)
            t = t + conv(mid, f"{prefix}.{i}.res.2.weight", padding=1)
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
        t = F.conv_transpose2d(_q(t + skips[lvl], round_bf16), w(f"m_up{lvl}.0.weight"), stride=2)
        t = blocks(t, f"m_up{lvl}", 1)
    return conv(t + skips[0], "m_tail.weight", padding=1)


def preactivation_signs_ref(sd, x, sigma, dtype, round_bf16=False):
    """[pre-activation > 0] of every ResBlock of the plain forward, in network order."""
    signs = []
    with torch.no_grad():
        masked_network_ref(sd, x, sigma, None, dtype, round_bf16, signs)
    return signs


def vjp_ref(sd, masks, g, dtype, round_bf16=False):
    """J^T g of masked_network_ref with respect to x: with the masks fixed the network is linear in (x, sigma), so its
    transpose does not depend on x. Written out layer by layer from the forward weights; with round_bf16 the weights and
    the input of every transposed convolution go through bfloat16 and everything else stays in `dtype`, as in the forward."""
    nb = _nb(sd)
    w = lambda key: _q(sd[key].to(dtype), round_bf16)          # noqa: E731
    conv3_t = lambda t, key: F.conv_transpose2d(_q(t, round_bf16), w(key), padding=1)      # noqa: E731
    it = reversed(list(masks))

    def blocks_t(t, prefix, first):
        for i in reversed(range(first, first + nb)):
            gm = conv3_t(t, f"{prefix}.{i}.res.2.weight") * next(it).to(dtype)
            t = t + conv3_t(gm, f"{prefix}.{i}.res.0.weight")
        return t

    t = conv3_t(g.to(dtype), "m_tail.weight")
    skips = {0: t}                                              # the gradient each U-Net skip carries, by level
    for lvl in (1, 2, 3):
        t = blocks_t(t, f"m_up{lvl}", 1)
        t = F.conv2d(_q(t, round_bf16), w(f"m_up{lvl}.0.weight"), stride=2)
        skips[lvl] = t
    t = blocks_t(t, "m_body", 0) + skips[3]
    for lvl in (3, 2, 1):
        t = F.conv_transpose2d(_q(t, round_bf16), w(f"m_down{lvl}.{nb}.weight"), stride=2)
        t = blocks_t(t, f"m_down{lvl}", 0) + skips[lvl - 1]
    return conv3_t(t, "m_head.weight")[:, :3]


def masked_denoiser_ref(sd, masks, dtype, round_bf16=False):
    """D(aux, sigma) for dps_step_ref: masked_network_ref forward, vjp_ref backward (so that round_bf16 rounds the backward
    pass where the kernels do, which autograd through the forward's roundings would not)."""

    class Net(torch.autograd.Function):
        @staticmethod
        def forward(ctx, aux, sigma):
            with torch.no_grad():
                return masked_network_ref(sd, aux, sigma, masks, dtype, round_bf16)

        @staticmethod
        def backward(ctx, g):
            with torch.no_grad():
                return vjp_ref(sd, masks, g, dtype, round_bf16), None

    return lambda aux, sigma: Net.apply(aux, sigma)


def mask_flips(masks, signs):
    """The number of units where the two lists of bool tensors differ."""
    return sum(int((m.cpu() != s.cpu()).sum()) for m, s in zip(masks, signs))
