"""GPU: the sei_adm_* kernels one by one -- the biased convolution against float64 F.conv2d with a derived accumulation bound,
GroupNorm statistics / apply and attention against float64 within 4x the error of the float32 CPU chain --, the DiffUNet of
models/diffunet.py in both arithmetic modes against the float64 restatement of tests/diffunet_ref.py, the DiffPIR_DiffUNet
baseline against the float64 loop, determinism and batch independence, and test.py --model_kind DiffPIR_DiffUNet end to end."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import _native as N
import physics
import diffunet_ref as R
from models.diffpir import DiffPIRDiffUNet
from models.diffunet import DiffUNet
from test_pnp_baseline_gpu import (U16, U32, bf16_values, check, empty_grid, from_grid, image, pack, to_grid, trunk_grid)
from test_tv_baseline import blur_circ, gaussian_r2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAIRS = [(128, 128), (128, 256), (256, 256), (256, 512), (512, 512), (1024, 512), (768, 512), (768, 256), (512, 256),
         (384, 256), (384, 128), (256, 128)]
EXTENTS = [(1, 4, 5), (2, 9, 13), (1, 32, 40)]
CONV_CASES = [(ci, co, e) for ci, co in PAIRS for e in EXTENTS] + [(512, 512, (2, 1, 1)), (1024, 512, (2, 1, 1))]


# ---- the convolution ----

@pytest.mark.parametrize("Cin,Cout,ext", CONV_CASES)
def test_conv3x3_bias_and_residual(Cin, Cout, ext):
    """42, 330 and 1428 grid rows (below one tile, not a tile multiple, several tiles) and the 1 x 1 image of the deepest
    level, where every tap but the centre reads border. Operands are bf16-exact, so the only error is the float32
    accumulation, |err| <= 9 Cin 2^-24 conv(|x|, |w|), plus 2^-23 (|conv| + |bias| + |res|) for the float32 additions, plus
    2^-8 |ref| for a bf16 result."""
    B, H, W = ext
    x = bf16_values((B, Cin, H, W), Cin + H)
    w = bf16_values((Cout, Cin, 3, 3), Cout + W, scale=math.sqrt(1.0 / (9 * Cin)))
    bias = bf16_values((Cout,), 7, scale=0.5)
    res = bf16_values((B, Cout, H, W), 3)
    conv = F.conv2d(x, w, padding=1)
    acc = 9 * Cin * U32 * F.conv2d(x.abs(), w.abs(), padding=1)
    b4 = bias[None, :, None, None]
    xg, guard = to_grid(x)
    wt, bg = pack(w), bias.float().cuda()
    # bias -> float32
    tg, _ = empty_grid(B, Cout, H, W, torch.float32)
    N.call("sei_adm_conv", xg[guard:].data_ptr(), wt.data_ptr(), bg.data_ptr(), Cin, Cout, 9, B, H, W, None, tg.data_ptr(), None)
    got, clean = from_grid(tg, 0, B, Cout, H, W)
    check(f"conv {Cin}->{Cout} {ext} bias", got, conv + b4, acc + 2 * U32 * (conv.abs() + b4.abs()))
    assert clean
    # bias + residual -> float32 and bf16
    rg = trunk_grid(res)
    t2, _ = empty_grid(B, Cout, H, W, torch.float32)
    y2, g2 = empty_grid(B, Cout, H, W, torch.bfloat16)
    N.call("sei_adm_conv", xg[guard:].data_ptr(), wt.data_ptr(), bg.data_ptr(), Cin, Cout, 9, B, H, W, rg.data_ptr(),
           t2.data_ptr(), y2[g2:].data_ptr())
    ref = conv + b4 + res
    bound = acc + 2 * U32 * (conv.abs() + b4.abs() + res.abs())
    got32, c32 = from_grid(t2, 0, B, Cout, H, W)
    got16, c16 = from_grid(y2, g2, B, Cout, H, W)
    check(f"conv {Cin}->{Cout} {ext} bias + residual f32", got32, ref, bound)
    check(f"conv {Cin}->{Cout} {ext} bias + residual bf16", got16, ref, bound + U16 * ref.abs())
    assert c32 and c16                                       # borders zero, guard rows untouched
    assert from_grid(xg, guard, B, Cin, H, W)[1]             # the input grid was only read
    assert torch.equal(rg, trunk_grid(res))
    # the same bits on a second run, and in place on the residual
    t3, _ = empty_grid(B, Cout, H, W, torch.float32)
    N.call("sei_adm_conv", xg[guard:].data_ptr(), wt.data_ptr(), bg.data_ptr(), Cin, Cout, 9, B, H, W, rg.data_ptr(),
           t3.data_ptr(), None)
    assert torch.equal(t3, t2)
    N.call("sei_adm_conv", xg[guard:].data_ptr(), wt.data_ptr(), bg.data_ptr(), Cin, Cout, 9, B, H, W, rg.data_ptr(),
           rg.data_ptr(), None)
    assert torch.equal(rg, t2)
    if B > 1:                                                # image 1 alone gives the bits it has in the batch
        x1, g1 = to_grid(x[1:])
        t1, _ = empty_grid(1, Cout, H, W, torch.float32)
        N.call("sei_adm_conv", x1[g1:].data_ptr(), wt.data_ptr(), bg.data_ptr(), Cin, Cout, 9, 1, H, W, None, t1.data_ptr(), None)
        rows = (H + 2) * (W + 2)
        assert torch.equal(t1, tg[rows:])


@pytest.mark.parametrize("Cin,Cout", [(768, 512), (384, 128), (512, 1536)])
def test_conv1x1(Cin, Cout):
    """The 1x1 skips and attention's projections: one tap, no guard rows read."""
    B, H, W = 2, 5, 7
    x = bf16_values((B, Cin, H, W), Cin)
    w = bf16_values((Cout, Cin, 1, 1), Cout, scale=math.sqrt(1.0 / Cin))
    bias = bf16_values((Cout,), 8, scale=0.5)
    ref = F.conv2d(x, w) + bias[None, :, None, None]
    bound = Cin * U32 * F.conv2d(x.abs(), w.abs()) + 2 * U32 * ref.abs() + 2 * U32 * bias.abs()[None, :, None, None]
    xg, guard = to_grid(x)
    xg[:guard] = float("nan")                                # a read of a guard row would show
    xg[-guard:] = float("nan")
    tg, _ = empty_grid(B, Cout, H, W, torch.float32)
    yg, g2 = empty_grid(B, Cout, H, W, torch.bfloat16)
    wt, bg = pack(w), bias.float().cuda()                    # (held: a temporary's memory could be handed out again)
    N.call("sei_adm_conv", xg[guard:].data_ptr(), wt.data_ptr(), bg.data_ptr(), Cin, Cout, 1, B, H, W, None, tg.data_ptr(),
           yg[g2:].data_ptr())
    got32, c32 = from_grid(tg, 0, B, Cout, H, W)
    got16, c16 = from_grid(yg, g2, B, Cout, H, W)
    check(f"conv1x1 {Cin}->{Cout} f32", got32, ref, bound)
    check(f"conv1x1 {Cin}->{Cout} bf16", got16, ref, bound + U16 * ref.abs())
    assert c32 and c16


def test_head_and_tail():
    """The head 3 -> 128 from the NCHW image (rounded to bf16 like every convolution input) and the tail 128 -> 3 to NCHW."""
    B, H, W = 2, 9, 13
    x = bf16_values((B, 3, H, W), 21)
    w = bf16_values((128, 3, 3, 3), 22, scale=math.sqrt(1.0 / 27))
    bias = bf16_values((128,), 23, scale=0.5)
    ref = F.conv2d(x, w, bias, padding=1)
    bound = 27 * U32 * F.conv2d(x.abs(), w.abs(), padding=1) + 2 * U32 * (ref.abs() + bias.abs()[None, :, None, None])
    rows, guard = B * (H + 2) * (W + 2), W + 3
    g = torch.full((rows + 2 * guard, 32), 3.0, dtype=torch.bfloat16, device="cuda")
    xg = x.float().cuda()
    N.call("sei_adm_pack_image", xg.data_ptr(), g[guard:].data_ptr(), B, H, W)
    packed, clean = from_grid(g, guard, B, 32, H, W)
    assert clean and torch.equal(packed[:, :3], x) and float(packed[:, 3:].abs().max()) == 0.0
    tg, _ = empty_grid(B, 128, H, W, torch.float32)
    wt, bg = pack(F.pad(w, (0, 0, 0, 0, 0, 29))), bias.float().cuda()
    N.call("sei_adm_conv", g[guard:].data_ptr(), wt.data_ptr(), bg.data_ptr(), 32, 128, 9, B, H, W, None, tg.data_ptr(), None)
    got, c32 = from_grid(tg, 0, B, 128, H, W)
    check("head", got, ref, bound)
    assert c32

    z = bf16_values((B, 128, H, W), 24)
    w3 = bf16_values((3, 128, 3, 3), 25, scale=math.sqrt(1.0 / (9 * 128)))
    b3 = bf16_values((3,), 26, scale=0.5)
    ref = F.conv2d(z, w3, b3, padding=1)
    bound = 9 * 128 * U32 * F.conv2d(z.abs(), w3.abs(), padding=1) + 2 * U32 * (ref.abs() + b3.abs()[None, :, None, None])
    zg, guard = to_grid(z)
    out = torch.full((B, 3, H, W), 9.0, device="cuda")
    wt, bg = pack(F.pad(w3, (0, 0, 0, 0, 0, 0, 0, 13))), F.pad(b3, (0, 13)).float().cuda()
    N.call("sei_adm_tail", zg[guard:].data_ptr(), wt.data_ptr(), bg.data_ptr(), 128, B, H, W, out.data_ptr())
    check("tail", out.cpu().double(), ref, bound)


# ---- GroupNorm ----

SPLITS = {128: (128, 0), 256: (128, 128), 384: (256, 128), 512: (256, 256), 768: (512, 256), 1024: (512, 512)}
GN_EXTENTS = [(2, 1, 1), (2, 2, 3), (1, 9, 13), (1, 32, 40)]
SAME, DOWN, UP = 0, 1, 2


def _resample64(v, how):
    if how == DOWN:
        return F.avg_pool2d(v, 2)
    if how == UP:
        return v.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    return v


def _gn_chain(x, gamma, beta, mod, how, dtype):
    """The two-pass chain in `dtype`: (mean, rstd, SiLU(GN(x) [(1 + scale) + shift]) resampled)."""
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    B, C = x.shape[:2]
    g = x.reshape(B, 32, -1)
    mean = g.mean(-1, keepdim=True)
    var = ((g - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    v = ((g - mean) * rstd).reshape(x.shape) * gamma[None, :, None, None] + beta[None, :, None, None]
    if mod is not None:
        mod = mod.to(dtype)
        v = v * (1 + mod[:, :C, None, None]) + mod[:, C:, None, None]
    return mean[..., 0], rstd[..., 0], _resample64(F.silu(v), how)


def _gn_run(x32, Ca, Cb, gamma, beta, mod, how, want16, want32):
    """The kernels on float32 NCHW x32 split into two trunks at Ca: (stats, bf16 result or None, float32 result or None,
    grids clean)."""
    B, C, H, W = x32.shape
    xa = trunk_grid(x32[:, :Ca].double())
    xb = trunk_grid(x32[:, Ca:].double()) if Cb else None
    st = torch.full((B, 32, 2), 9.0, device="cuda")
    nfl = N.lib().sei_adm_gn_part_floats(H, W)
    assert nfl == 64 * -(-H * W // 1024)                      # slices of 1024 pixels: (1, 32, 40) and its resamplings have several
    part = torch.full((B * nfl,), 9.0, device="cuda")
    N.call("sei_adm_gn_stats", xa.data_ptr(), Ca, N.ptr(xb), Cb, B, H, W, 1e-5, st.data_ptr(), part.data_ptr())
    Ho, Wo = (H // 2, W // 2) if how == DOWN else (2 * H, 2 * W) if how == UP else (H, W)
    y16, g16 = empty_grid(B, C, Ho, Wo, torch.bfloat16)
    y32, _ = empty_grid(B, C, Ho, Wo, torch.float32)
    gg, bg, mg = gamma.float().cuda(), beta.float().cuda(), None if mod is None else mod.float().cuda()
    N.call("sei_adm_gn_apply", xa.data_ptr(), Ca, N.ptr(xb), Cb, st.data_ptr(), gg.data_ptr(), bg.data_ptr(), N.ptr(mg), 1, B, H,
           W, how, y16[g16:].data_ptr() if want16 else None, y32.data_ptr() if want32 else None)
    got16, c16 = from_grid(y16, g16, B, C, Ho, Wo)
    got32, c32 = from_grid(y32, 0, B, C, Ho, Wo)
    return st.cpu().double(), got16 if want16 else None, got32 if want32 else None, c16 and c32


@pytest.mark.parametrize("ext", GN_EXTENTS)
@pytest.mark.parametrize("C", sorted(SPLITS))
def test_groupnorm_stats_and_apply(C, ext):
    """Every width (the seam cases from two trunks: at 384 and 768 a group straddles the seam), every extent (for the 2x2
    average the listed extents are the OUTPUT's), with and without modulation, each resampling, bf16 and float32 outputs,
    on a unit-scale input and on one of mean 100 and standard deviation 1. Bound: 4x the error of the float32 two-pass CPU
    chain against float64, relative to the float64 result's max-abs (statistics: to the largest |mean| and rstd); a bf16
    result adds 2^-8 |ref|."""
    B, H, W = ext
    Ca, Cb = SPLITS[C]
    g = torch.Generator().manual_seed(C + H)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    mod = 0.3 * torch.randn((B, 2 * C), generator=g)
    for offset in (0.0, 100.0):
        for how in (SAME, DOWN, UP):
            hi, wi = (2 * H, 2 * W) if how == DOWN else (H, W)
            x32 = (offset + torch.randn((B, C, hi, wi), generator=g)).float()
            for m in (None, mod):
                mean64, rstd64, ref = _gn_chain(x32, gamma, beta, m, how, torch.float64)
                mean32, rstd32, cpu = _gn_chain(x32, gamma, beta, m, how, torch.float32)
                scale = float(ref.abs().max())
                e_cpu = float((cpu.double() - ref).abs().max()) / scale
                e_mean = float((mean32.double() - mean64).abs().max()) / max(float(mean64.abs().max()), 1.0)
                e_rstd = float((rstd32.double() - rstd64).abs().max()) / float(rstd64.max())
                st, got16, got32, clean = _gn_run(x32, Ca, Cb, gamma, beta, m, how, True, True)
                g_mean = float((st[..., 0] - mean64).abs().max()) / max(float(mean64.abs().max()), 1.0)
                g_rstd = float((st[..., 1] - rstd64).abs().max()) / float(rstd64.max())
                e32 = float((got32 - ref).abs().max()) / scale
                e16 = float(((got16 - ref).abs() - U16 * ref.abs()).max()) / scale
                print(f"GN C={C} {ext} offset={offset:g} how={how} mod={m is not None}: mean {g_mean:.2e} ({e_mean:.2e}), rstd "
                      f"{g_rstd:.2e} ({e_rstd:.2e}), f32 {e32:.2e}, bf16 beyond its rounding {e16:.2e} (cpu {e_cpu:.2e})")
                assert clean
                assert g_mean <= 4 * max(e_mean, U32) and g_rstd <= 4 * max(e_rstd, U32)
                assert e32 <= 4 * e_cpu and e16 <= 4 * e_cpu
    # one output at a time gives the same bits; image 1 of the batch equals the same image run alone
    st, got16, got32, _ = _gn_run(x32, Ca, Cb, gamma, beta, mod, UP, True, True)
    _, only16, _, _ = _gn_run(x32, Ca, Cb, gamma, beta, mod, UP, True, False)
    _, _, only32, _ = _gn_run(x32, Ca, Cb, gamma, beta, mod, UP, False, True)
    assert torch.equal(only16, got16) and torch.equal(only32, got32)
    if B > 1:
        st1, a16, a32, _ = _gn_run(x32[1:], Ca, Cb, gamma, beta, mod[1:], UP, True, True)
        assert torch.equal(st1[0], st[1]) and torch.equal(a16[0], got16[1]) and torch.equal(a32[0], got32[1])


def test_plain_resampling_of_the_skip_path():
    """Without statistics the apply kernel is R(x): the copy (as the bf16 grid the 1x1 skip reads), the 2x2 average and the
    2x repetition, from one trunk or two."""
    B, H, W = 2, 4, 6
    x32 = torch.randn((B, 384, H, W), generator=torch.Generator().manual_seed(9)).float()
    xa, xb = trunk_grid(x32[:, :256].double()), trunk_grid(x32[:, 256:].double())
    for how in (SAME, DOWN, UP):
        Ho, Wo = (H // 2, W // 2) if how == DOWN else (2 * H, 2 * W) if how == UP else (H, W)
        y16, g16 = empty_grid(B, 384, Ho, Wo, torch.bfloat16)
        y32, _ = empty_grid(B, 384, Ho, Wo, torch.float32)
        N.call("sei_adm_gn_apply", xa.data_ptr(), 256, xb.data_ptr(), 128, None, None, None, None, 0, B, H, W, how,
               y16[g16:].data_ptr(), y32.data_ptr())
        ref = _resample64(x32.double(), how)
        got32, c32 = from_grid(y32, 0, B, 384, Ho, Wo)
        got16, c16 = from_grid(y16, g16, B, 384, Ho, Wo)
        assert c32 and c16
        assert float((got32 - ref).abs().max()) <= 2 * U32 * float(ref.abs().max())
        assert torch.equal(got16, got32.to(torch.bfloat16).double())
        if how != DOWN:
            assert torch.equal(got32, ref)


# ---- attention ----

def _attention_case(B, H, W, C, spread, seed):
    """qkv (B, 3C, T) bf16-exact float64; q and k at `spread` so that the scores (q . k) / 8 have that variance."""
    T = H * W
    qkv = bf16_values((B, 3 * C, T), seed)
    heads = C // 64
    v = qkv.reshape(B, heads, 3, 64, T).clone()
    v[:, :, :2] = (v[:, :, :2] * spread).to(torch.bfloat16).double()
    return v.reshape(B, 3 * C, T)


def _attention_chain(qkv, dtype, round_p):
    B, C3, T = qkv.shape
    heads = C3 // 192
    q, k, v = qkv.to(dtype).reshape(B * heads, 192, T).split(64, dim=1)
    s = torch.einsum("bct,bcs->bts", q, k) * 0.125
    p = torch.softmax(s, dim=-1)
    if round_p:
        p = p.to(torch.bfloat16).to(dtype)
    a = torch.einsum("bts,bcs->bct", p, v).reshape(B, C3 // 3, T)
    return (a.to(torch.bfloat16).to(dtype) if round_p else a), float(s.abs().max())


def _attention_run(qkv, B, H, W, C):
    grid = F.pad(qkv.reshape(B, 3 * C, H, W).permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1)).reshape(-1, 3 * C)
    qg = grid.to(torch.bfloat16).cuda()
    out = torch.zeros((qg.shape[0], C), dtype=torch.bfloat16, device="cuda")
    N.call("sei_adm_attention", qg.data_ptr(), C, B, H, W, out.data_ptr())
    body = out.cpu().double().view(B, H + 2, W + 2, C)
    border = body.clone()
    border[:, 1:-1, 1:-1] = 0
    return body[:, 1:-1, 1:-1].permute(0, 3, 1, 2).reshape(B, C, H * W), float(border.abs().max()) == 0.0, out


@pytest.mark.parametrize("H,W,spread", [(1, 1, 1.0), (2, 2, 1.0), (2, 3, 1.0), (8, 8, 1.0), (16, 17, 1.0), (8, 8, 4.7), (16, 17, 4.7)])
def test_attention(H, W, spread):
    """C = 512 (8 heads), B = 2, T = 1, 4, 6, 64 and 272 (no multiple of the 32-key tile or of the 16-query block). With
    spread 4.7 the scores have standard deviation 22 and reach magnitudes of 80 to 120: a softmax without the row maximum overflows. Bound: 4x the
    error of the float32 CPU chain with the same roundings (bf16 probabilities, a bf16 result) against float64."""
    B, C = 2, 512
    qkv = _attention_case(B, H, W, C, spread, 31 + H * W)
    ref, smax = _attention_chain(qkv, torch.float64, False)
    cpu, _ = _attention_chain(qkv, torch.float32, True)
    if spread > 1 and H * W > 4:
        assert smax > 89                                     # exp overflows float32 without the maximum
    scale = float(ref.abs().max())
    e_cpu = float((cpu.double() - ref).abs().max()) / scale
    got, clean, raw = _attention_run(qkv, B, H, W, C)
    e_gpu = float((got - ref).abs().max()) / scale
    print(f"attention T={H * W} spread={spread:g}: {e_gpu:.2e} (bf16-rounded float32 cpu {e_cpu:.2e}), largest score {smax:.1f}")
    assert clean and bool(torch.isfinite(got).all())
    assert e_gpu <= 4 * e_cpu
    _, _, again = _attention_run(qkv, B, H, W, C)
    assert torch.equal(again, raw)
    alone, _, _ = _attention_run(qkv[1:], 1, H, W, C)
    assert torch.equal(alone[0], got[1])


# ---- the network ----

@pytest.fixture(scope="module")
def net():
    sd = R.synthetic_state_dict(seed=0)
    model = DiffUNet()
    model.load_state_dict(sd)
    return sd, model.cuda().eval()


@pytest.mark.parametrize("sigma", [0.02, 0.5])
@pytest.mark.parametrize("shape", [(2, 3, 32, 32), (1, 3, 32, 64), (1, 3, 64, 96)])
def test_network_matches_float64_restatement(net, shape, sigma):
    """sigma 0.02 and 0.5 map to t = 8 and t = 258. Max-norm error relative to the float64 result's max-abs, on the noise
    estimate (ahead of the clamp, which hides errors) and on the denoiser's result: the f32 mode at most 4x that of the
    float32 CPU chain, the bf16 mode at most 4x that of the float32 CPU chain with the bf16 mode's roundings. Both modes give
    the same bits on a second run."""
    sd, model = net
    x = image(shape, seed=shape[-1])
    t, s, alpha = R.timestep_ref(sigma)
    assert t == {0.02: 8, 0.5: 258}[sigma]
    R.assert_activation_range(sd, math.sqrt(alpha) * (2 * x - 1), t)
    refs = {k: R.denoise_ref(sd, x, sigma, dt, rb, return_eps=True) for k, dt, rb in (("f64", torch.float64, False), ("f32", torch.float32, False), ("bf16", torch.float32, True))}
    for mode in ("f32", "bf16"):
        model.compute_dtype = mode
        eps = model.eps(x.cuda(), sigma)[0]
        out = model(x.cuda(), sigma)
        assert out.shape == x.shape and out.dtype == torch.float32
        assert torch.equal(model.eps(x.cuda(), sigma)[0], eps) and torch.equal(model(x.cuda(), sigma), out)
        for name, got, i in (("eps", eps, 0), ("result", out, 1)):
            ref = refs["f64"][i]
            scale = float(ref.abs().max())
            e_gpu = float((got.cpu().double() - ref).abs().max()) / scale
            e_cpu = float((refs[mode][i].double() - ref).abs().max()) / scale
            print(f"DiffUNet {shape} sigma={sigma} {mode} mode, {name}: {e_gpu:.2e} (cpu chain {e_cpu:.2e}), max-abs {scale:.3f}")
            assert e_gpu <= 4 * e_cpu, (mode, name)
    model.compute_dtype = "bf16"
    assert 0.0 <= float(out.min()) and float(out.max()) <= 1.0


def test_network_is_batch_independent_and_checks_its_input(net):
    sd, model = net
    x = image((3, 3, 32, 64), seed=7).cuda()
    for mode in ("bf16", "f32"):
        model.compute_dtype = mode
        whole = model.eps(x, 0.1)[0].clone()
        for i in (0, 2):
            assert torch.equal(model.eps(x[i:i + 1].contiguous(), 0.1)[0][0], whole[i]), (mode, i)
    model.compute_dtype = "bf16"
    with pytest.raises(TypeError):
        model(x.double(), 0.1)
    with pytest.raises(TypeError):
        model(x.cpu(), 0.1)
    with pytest.raises(ValueError, match="32"):
        model(x[..., :40].contiguous(), 0.1)
    with pytest.raises(ValueError):
        model(x, 0.0)


# ---- DiffPIR end to end ----

class Noise:
    sigma = 5 / 255


def _case(kind):
    """(y, operator, A, At, padded measurement extents): the float64 operators act on the padded extents."""
    g = torch.Generator().manual_seed(4)
    if kind == "deblurring":
        y = torch.rand((1, 3, 40, 56), generator=g, dtype=torch.float64)              # pads to 64 x 64
        k = gaussian_r2()
        op = physics.BlurV2(kernel=physics.get_kernel("Gaussian_R2")[None, None].cuda())
        A = lambda dt: (lambda v: blur_circ(v, k.to(dt)))                       # noqa: E731
        At = lambda dt: (lambda v: blur_circ(v, k.to(dt), transpose=True))      # noqa: E731
        op.task = "deblurring"
        return y, op, A, At, (64, 64)
    from physics import _bands
    op = physics.Downsampling(rate=2, antialias=True)
    op.task = "sr"
    y = torch.rand((1, 3, 24, 40), generator=g, dtype=torch.float64)                  # pads to 32 x 48, output 48 x 80
    dv, dh = (torch.from_numpy(np.asarray(_bands.aa_bicubic_matrix(n, 1 / 2), dtype=np.float64)) for n in (64, 96))
    uv, uh = (torch.from_numpy(np.asarray(_bands.plain_bicubic_matrix(n, 2), dtype=np.float64)) for n in (32, 48))
    A = lambda dt: (lambda v: dv.to(dt) @ v @ dh.to(dt).T)                      # noqa: E731
    At = lambda dt: (lambda v: uv.to(dt) @ v @ uh.to(dt).T)                     # noqa: E731  (the reference's adjoint)
    return y, op, A, At, (32, 48)


@pytest.mark.parametrize("kind", ["deblurring", "sr"])
def test_diffpir_diffunet_matches_float64_loop(net, kind):
    """A 5-iteration schedule, cg_tol = 0 and cg_max_iter = 12 so that both sides run the same iteration counts, the same
    noise tensors on both sides through `draw`. f32 mode: the error against the float64 loop is at most 4x that of the
    float32 CPU loop. bf16 mode: finite, and within 4x the distance that the bf16 roundings move the float32 CPU loop.
    The result has rate x the unpadded extents."""
    sd, model = net
    y, op, A, At, padded = _case(kind)
    op.noise_model = Noise()
    rate = 2 if kind == "sr" else 1
    x_shape = (1, 3, rate * padded[0], rate * padded[1])
    draws = {i: torch.randn(x_shape, generator=torch.Generator().manual_seed(100 + i), dtype=torch.float64) for i in range(6)}
    kw = dict(max_iter=5, cg_max_iter=12, cg_tol=0.0)
    den = lambda dt, rb: (lambda v, s: R.denoise_ref(sd, v, s, dt, rb))         # noqa: E731
    run = lambda dt, rb: R.diffpir_diffunet_ref(y, A(dt), At(dt), den(dt, rb), Noise.sigma, dt, draws,   # noqa: E731
                                                kind == "deblurring", rate, **kw)
    ref, cpu32, cpu16 = run(torch.float64, False), run(torch.float32, False), run(torch.float32, True)
    scale = float(ref.abs().max())
    assert ref.shape == (1, 3, rate * y.shape[2], rate * y.shape[3])

    class Fixed(DiffPIRDiffUNet):
        def draw(self, i, like):
            return draws[i].float().to(like.device)

    wrapper = Fixed(op, model, **kw)
    assert wrapper.task == op.task and len(wrapper.state_dict()) == 0
    out = {}
    for mode in ("f32", "bf16"):
        model.compute_dtype = mode
        out[mode] = wrapper(y.float().cuda()).cpu().double()
        assert out[mode].shape == ref.shape and wrapper.cg_iterations == [12] * 4
    model.compute_dtype = "bf16"
    e_gpu = float((out["f32"] - ref).abs().max()) / scale
    e_cpu = float((cpu32.double() - ref).abs().max()) / scale
    d_gpu = float((out["bf16"] - out["f32"]).abs().max()) / scale
    d_cpu = float((cpu16.double() - cpu32.double()).abs().max()) / scale
    print(f"DiffPIR_DiffUNet {kind}: f32 mode {e_gpu:.2e} (float32 cpu {e_cpu:.2e}); bf16 - f32: {d_gpu:.2e} (cpu loop "
          f"{d_cpu:.2e}); relative to max-abs {scale:.3f}")
    assert e_gpu <= 4 * e_cpu
    assert bool(torch.isfinite(out["bf16"]).all()) and d_gpu <= 4 * d_cpu


# ---- the driver ----

@pytest.fixture(scope="module")
def weights_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("diffunet") / "diffunet_synthetic.pth")
    torch.save(R.synthetic_state_dict(seed=0), path)
    return path


COMMON = ["--device", "cuda", "--dataset", "synthetic", "--indices", "0", "--model_kind", "DiffPIR_DiffUNet",
          "--diffpir_iterations", "3"]


def run_test_py(*flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), *COMMON, *flags], capture_output=True, text=True,
                          timeout=300)


@pytest.mark.parametrize("task", [["--task", "deblurring", "--kernel", "Gaussian_R2"], ["--task", "sr", "--sr_factor", "2"]])
def test_test_py_runs_the_baseline(weights_file, task):
    r = run_test_py(*task, "--diffunet_weights", weights_file)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert "N: 1" in lines
    assert math.isfinite(float([ln for ln in lines if ln.startswith("PSNR:")][0].split()[-1]))


def test_test_py_names_the_missing_flag():
    r = run_test_py("--task", "deblurring", "--kernel", "Gaussian_R2")
    assert r.returncode != 0 and "--diffunet_weights" in r.stderr
