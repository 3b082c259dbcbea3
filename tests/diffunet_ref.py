"""Float64 / float32 restatement of the diffusion U-Net of the DiffPIR_DiffUNet baseline (guided-diffusion's "ADM" network as
deepinv 0.2's DiffUNet(large_model=False) builds it: 128 base channels, multipliers (1, 1, 2, 2, 4, 4), one ResBlock per
level, resampling ResBlocks, 64-wide attention heads in the legacy qkv order at 1/16 resolution and in the middle), of the
denoiser call around it and of the DiffPIR loop and the reference's pad-and-crop wrapper: the pinned truth of
tests/test_diffunet_baseline.py and tests/test_diffunet_baseline_gpu.py. Written from the published architecture,
independently of models/diffunet.py. Not collected."""
import math

import torch
from torch import nn
from torch.nn import functional as F

from diffpir_ref import nearest_ref, schedule_ref, tables_ref
from drunet_ref import cg_ref

CH, MULT, EMB, HEAD_DIM, ATTN_DS = 128, (1, 1, 2, 2, 4, 4), 512, 64, 16


class RB(nn.Module):
    def __init__(self, cin, cout, resample=None):
        super().__init__()
        self.resample = resample
        self.in_layers = nn.Sequential(nn.GroupNorm(32, cin), nn.SiLU(), nn.Conv2d(cin, cout, 3, padding=1))
        self.emb_layers = nn.Sequential(nn.SiLU(), nn.Linear(EMB, 2 * cout))
        self.out_layers = nn.Sequential(nn.GroupNorm(32, cout), nn.SiLU(), nn.Dropout(0.0), nn.Conv2d(cout, cout, 3, padding=1))
        self.skip_connection = nn.Identity() if cin == cout else nn.Conv2d(cin, cout, 1)


class Attn(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.norm = nn.GroupNorm(32, c)
        self.qkv = nn.Conv1d(c, 3 * c, 1)
        self.proj_out = nn.Conv1d(c, c, 1)


class DiffUNetRef(nn.Module):
    """The module tree with guided-diffusion's names; used for its key list, the arithmetic is `network_ref`."""

    def __init__(self):
        super().__init__()
        self.time_embed = nn.Sequential(nn.Linear(CH, EMB), nn.SiLU(), nn.Linear(EMB, EMB))
        self.input_blocks = nn.ModuleList([nn.Sequential(nn.Conv2d(3, CH, 3, padding=1))])
        widths, ch, ds = [CH], CH, 1
        for level, m in enumerate(MULT):
            layers = [RB(ch, m * CH)]
            ch = m * CH
            if ds == ATTN_DS:
                layers.append(Attn(ch))
            self.input_blocks.append(nn.Sequential(*layers))
            widths.append(ch)
            if level != len(MULT) - 1:
                self.input_blocks.append(nn.Sequential(RB(ch, ch, "down")))
                widths.append(ch)
                ds *= 2
        self.middle_block = nn.Sequential(RB(ch, ch), Attn(ch), RB(ch, ch))
        self.output_blocks = nn.ModuleList()
        for level, m in list(enumerate(MULT))[::-1]:
            for i in range(2):
                layers = [RB(ch + widths.pop(), m * CH)]
                ch = m * CH
                if ds == ATTN_DS:
                    layers.append(Attn(ch))
                if level and i == 1:
                    layers.append(RB(ch, ch, "up"))
                    ds //= 2
                self.output_blocks.append(nn.Sequential(*layers))
        self.out = nn.Sequential(nn.GroupNorm(32, CH), nn.SiLU(), nn.Conv2d(CH, 6, 3, padding=1))


def _q(t, on):
    """Through bfloat16 and back (round to nearest even) when `on`."""
    return t.to(torch.bfloat16).to(t.dtype) if on else t


def timestep_embedding_ref(t, dtype=torch.float64):
    """cat(cos(t f), sin(t f)), f_i = exp(-ln(10000) i / 64), i < 64: a (1, 128) tensor."""
    f = torch.exp(-math.log(10000.0) * torch.arange(64, dtype=dtype) / 64)
    a = float(t) * f
    return torch.cat([torch.cos(a), torch.sin(a)])[None]


def network_ref(sd, z, t, dtype, round_bf16=False, trace=None):
    """eps = net(z, t)[:, :3] functionally from the state dict. With round_bf16 every matrix-product operand of the "bf16"
    mode goes through bfloat16 -- convolution and 1x1 inputs and weights, q, k, v, the softmax probabilities -- and nothing
    else does. `trace` (a list) collects the max-abs of every activation."""
    P = lambda key: sd[key].to(dtype)                             # noqa: E731
    W = lambda key: _q(sd[key].to(dtype), round_bf16)             # noqa: E731

    def note(v):
        if trace is not None:
            trace.append(float(v.abs().max()))
        return v

    def gn(v, key):
        return F.group_norm(v, 32, P(key + ".weight"), P(key + ".bias"), 1e-5)

    def conv(v, key, padding=1):
        return note(F.conv2d(_q(v, round_bf16), W(key + ".weight"), P(key + ".bias"), padding=padding))

    def resample(v, how):
        if how == "down":
            return F.avg_pool2d(v, 2)
        if how == "up":
            return v.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        return v

    def rb(v, key, how=None):
        cout = sd[key + ".in_layers.2.weight"].shape[0]
        h = conv(resample(F.silu(gn(v, key + ".in_layers.0")), how), key + ".in_layers.2")
        mod = F.linear(F.silu(emb), P(key + ".emb_layers.1.weight"), P(key + ".emb_layers.1.bias"))
        scale, shift = mod[:, :cout, None, None], mod[:, cout:, None, None]
        h = conv(F.silu(note(gn(h, key + ".out_layers.0") * (1 + scale) + shift)), key + ".out_layers.3")
        v = resample(v, how)
        if key + ".skip_connection.weight" in sd:
            v = conv(v, key + ".skip_connection", padding=0)
        return note(v + h)

    def attn(v, key):
        B, C, H, Wd = v.shape
        heads = C // HEAD_DIM
        n = gn(v, key + ".norm").reshape(B, C, H * Wd)
        qkv = note(F.conv1d(_q(n, round_bf16), W(key + ".qkv.weight"), P(key + ".qkv.bias")))
        q, k, val = (_q(p, round_bf16) for p in qkv.reshape(B * heads, 3 * HEAD_DIM, H * Wd).split(HEAD_DIM, dim=1))
        s = torch.einsum("bct,bcs->bts", q, k) * (1.0 / math.sqrt(HEAD_DIM))       # (q 64^-1/4) . (k 64^-1/4)
        p = _q(torch.softmax(s, dim=-1), round_bf16)
        a = note(torch.einsum("bts,bcs->bct", p, val).reshape(B, C, H * Wd))
        out = F.conv1d(_q(a, round_bf16), W(key + ".proj_out.weight"), P(key + ".proj_out.bias"))
        return note(v + out.reshape(B, C, H, Wd))

    def block(v, prefix):
        i = 0
        while f"{prefix}.{i}.in_layers.0.weight" in sd or f"{prefix}.{i}.norm.weight" in sd:
            key = f"{prefix}.{i}"
            if key + ".norm.weight" in sd:
                v = attn(v, key)
            else:
                how = None
                if prefix.startswith("input_blocks") and int(prefix.split(".")[1]) in (2, 4, 6, 8, 10):
                    how = "down"                                  # the ResBlock that stands alone between two levels
                if prefix.startswith("output_blocks") and i > 0:
                    how = "up"                                    # a second ResBlock of an output entry
                v = rb(v, key, how)
            i += 1
        return v

    z = z.to(dtype)
    e = timestep_embedding_ref(t, dtype)
    e = F.linear(e, P("time_embed.0.weight"), P("time_embed.0.bias"))
    emb = note(F.linear(F.silu(e), P("time_embed.2.weight"), P("time_embed.2.bias"))).expand(z.shape[0], -1)
    h = conv(z, "input_blocks.0.0")
    skips = [h]
    for n in range(1, 12):
        h = block(h, f"input_blocks.{n}")
        skips.append(h)
    h = block(h, "middle_block")
    for n in range(12):
        h = block(torch.cat([h, skips.pop()], 1), f"output_blocks.{n}")
    h = F.silu(gn(h, "out.0"))
    return note(F.conv2d(_q(h, round_bf16), W("out.2.weight")[:3], P("out.2.bias")[:3], padding=1))


def timestep_ref(sigma):
    """(t, s, alpha) of the denoiser call: the first timestep whose noise share sqrt(1 - ac[t]) is nearest to
    s = 2 sigma sqrt(alpha), alpha = 1 / (1 + 4 sigma^2)."""
    s1m = tables_ref()[1].double()
    alpha = 1.0 / (1.0 + 4.0 * sigma * sigma)
    s = 2.0 * sigma * math.sqrt(alpha)
    return int(torch.argmin((s1m - s).abs())), s, alpha


def denoise_ref(sd, x, sigma, dtype, round_bf16=False, return_eps=False):
    """The denoiser call forward(x, sigma) for x in [0, 1]; with return_eps, (the noise estimate, the result)."""
    sa = tables_ref()[0]
    t, s, alpha = timestep_ref(sigma)
    z = math.sqrt(alpha) * (2 * x.to(dtype) - 1)
    eps = network_ref(sd, z, t, dtype, round_bf16)
    out = ((z - s * eps) / float(sa[t])).clamp(-1, 1) / 2 + 0.5
    return (eps, out) if return_eps else out


def synthetic_state_dict(seed=0):
    """Random float32 weights with the real key set. First convolutions of a block, qkv, the head and the 1x1 skips at
    variance-preserving scale (std sqrt(1 / fan_in)); the tensors guided-diffusion zero-initialises are NOT left at zero:
    out_layers.3 and proj_out at half that scale (a block adds about half its input's spread), out.2 at full scale.
    GroupNorm weights 1 + 0.2 n, every bias 0.1 n, emb_layers weights at std 0.5 sqrt(1 / 512) so that scale and shift
    are of order 0.3."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, p in DiffUNetRef().state_dict().items():
        r = torch.randn(p.shape, generator=g)
        if key.endswith(".bias"):
            v = 0.1 * r
        elif p.dim() == 1:
            v = 1.0 + 0.2 * r
        else:
            fan_in = p[0].numel()
            std = math.sqrt(1.0 / fan_in)
            if ".out_layers.3." in key or ".proj_out." in key or ".emb_layers." in key:
                std *= 0.5
            v = std * r
        sd[key] = v.float()
    return sd


def assert_activation_range(sd, z, t, lo=1e-3, hi=1e3):
    """A condition on the fixture: the max-abs of every float64 activation lies in [lo, hi]."""
    trace = []
    network_ref(sd, z.double(), t, torch.float64, trace=trace)
    assert trace and lo <= min(trace) and max(trace) <= hi, (min(trace), max(trace))
    return min(trace), max(trace)


def pad_amounts(h, w, deblurring):
    m = 32 if deblurring else 16
    return (m - h % m) % m, (m - w % m) % m


def diffpir_diffunet_ref(y, A, At, denoiser, sigma, dtype, draws, deblurring, rate=1, max_iter=100, zeta=0.1, lambda_=7.0,
                         cg_max_iter=50, cg_tol=1e-3):
    """The reference wrapper's forward around deepinv's DiffPIR loop in `dtype`: reflect-pad y at the bottom and right,
    run the loop on the padded y (A / At act on the padded extents; `draws[i]` of the padded image's shape), crop to
    rate x the unpadded extents. `denoiser(x, sigma)` is a callable in `dtype`."""
    ph, pw = pad_amounts(y.shape[2], y.shape[3], deblurring)
    h, w = y.shape[2], y.shape[3]
    y = F.pad(y.to(dtype), (0, pw, 0, ph), mode="reflect")
    sa, s1m, red, srec = tables_ref()
    rhos, sigmas, seq = schedule_ref(sigma, lambda_, max_iter)
    Aty = At(y)
    x = 2 * Aty - 1
    x0 = None
    for i in range(len(seq)):
        cs = float(sigmas[seq[i]])
        t = nearest_ref(cs)
        at = 1.0 / float(srec[t]) ** 2
        if i == 0:
            x = (x + cs * draws[0].to(dtype)) / float(srec[-1])
        out = denoiser(x / (2 * math.sqrt(at)) + 0.5, cs / 2)
        x0 = (2 * out - 1).clamp(-1, 1)
        if not seq[i] == seq[-1]:
            gamma = 1.0 / (2.0 * float(rhos[t]))
            u = cg_ref(lambda v: At(A(v)) + v / gamma, Aty + (x0 / 2 + 0.5) / gamma, cg_max_iter, cg_tol)
            x0 = u * 2 - 1
            tn = nearest_ref(float(sigmas[seq[i + 1]]))
            eps = (x - float(sa[t]) * x0) / float(s1m[t])
            x = float(sa[tn]) * x0 + float(s1m[tn]) * (math.sqrt(1 - zeta) * eps + math.sqrt(zeta) * draws[i + 1].to(dtype))
    return (x0 / 2 + 0.5)[:, :, :rate * h, :rate * w]
