"""SwinIR window attention (sei_swin_attn_fwd / _bwd, exact f32; sei_swin_attn_fwd_bf16 / _bwd_bf16, MFMA) at the edges
tests/test_swinir_gpu.py leaves out: extents with a single window row or column (H == 8 or W == 8: every window is a
last-row window and wraps onto itself, what models/swinir.py runs on a thin image after its reflect padding), every
head shape and shift the entry points accept, fewer windows than a workgroup has waves, one and two heads, logits far
from O(1) with the FINITE -100 mask carrying probability mass, the value and layout of the stored log-sum-exp, the
`+=` contract of the bias-table gradient, and the whole network on 8-row images. The reference is the float64
restatement in tests/window_attention_ref.py (oracle/swinir_path.py's window_partition / shift_mask /
relative_position_index; the mask itself is held to the published calculate_mask in tests/test_host_logic.py)."""
import math

import numpy as np
import pytest
import torch

from oracle import swinir_path as sp
from window_attention_ref import _attention_reference, attention_logits

pytestmark = pytest.mark.gpu

HP = 32                                                     # the MFMA kernels' padded head width (30 -> 32)
GEOMS = [(1, 8, 8), (1, 8, 24), (2, 24, 8), (3, 8, 16), (1, 16, 8)]
GEOM_SHIFTS = [(g, s) for g in GEOMS for s in ((0, 4, 1, 3, 7) if g in ((1, 8, 24), (2, 24, 8)) else (0, 4))]
HEAD_SHAPES = [(1, 8), (2, 16), (1, 30), (6, 30), (3, 32)]


def relerr(a, b):
    a = a.detach().cpu().double().numpy()
    b = b.detach().cpu().double().numpy()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _gid(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) and not isinstance(v[0], tuple) else None


# ---------------------------------------------------------------------------------------------- exact-f32 kernels
def _f32_case(B, H, W, heads, hd, shift, qkv, table, go):
    """float64 reference (output, dqkv, dtable) and the f32 kernels' results on the same inputs."""
    from models import _swin_ops as S
    qd, td = qkv.double().requires_grad_(True), table.double().requires_grad_(True)
    ref = _attention_reference(qd, td, B, H, W, heads, shift)
    rq, rt = torch.autograd.grad(ref, [qd, td], go.double())
    out = S.window_attention(qkv.cuda(), table.cuda(), B, H, W, heads, shift)
    dtable = torch.zeros_like(table).cuda()
    dqkv = S.window_attention_bwd(qkv.cuda(), table.cuda(), go.cuda(), dtable, B, H, W, heads, shift)
    return (ref.detach(), rq, rt), (out, dqkv, dtable)


@pytest.mark.parametrize("heads,hd", HEAD_SHAPES)
@pytest.mark.parametrize("geom,shift", GEOM_SHIFTS, ids=lambda v: _gid(v) if isinstance(v, tuple) else f"s{v}")
def test_f32_window_attention_geometry_grid(geom, shift, heads, hd):
    """Forward, dqkv and dtable of the f32 kernels against float64 at test_window_attention_fwd_bwd's bars (5e-6 /
    2e-5, max-norm relative) on extents with ONE window along an axis, every shift parity class the region arithmetic
    of win_token distinguishes (0, 4, and 1 / 3 / 7 on the two extents with three windows along the other axis) and
    every head width the entry point accepts (8, 16, 30, 32), with 1, 2, 3 and 6 heads."""
    B, H, W = geom
    gen = torch.Generator().manual_seed(1000 * H + 10 * W + B + 100 * shift + hd + heads)
    C = heads * hd
    qkv = torch.randn((B * H * W, 3 * C), generator=gen)
    table = torch.randn((225, heads), generator=gen) * 0.5
    go = torch.randn((B * H * W, C), generator=gen)
    (ref, rq, rt), (out, dqkv, dtable) = _f32_case(B, H, W, heads, hd, shift, qkv, table, go)
    errs = relerr(out, ref), relerr(dqkv, rq), relerr(dtable, rt)
    print(f"f32 {geom} shift {shift} heads {heads} x {hd}: out {errs[0]:.2e} dqkv {errs[1]:.2e} dtable {errs[2]:.2e}")
    assert errs[0] < 5e-6, errs
    assert errs[1] < 2e-5 and errs[2] < 2e-5, errs


# ---------------------------------------------------------------------------------------------- bf16 MFMA kernels
def _pad_heads(x30, M, parts, heads):
    """(M, parts, heads, 30) float -> bf16 (M, parts * heads * 32) with zero pad lanes, as the packed qkv weights give."""
    x = torch.zeros((M, parts, heads, HP))
    x[..., :30] = x30
    return x.reshape(M, parts * heads * HP).bfloat16()


def _mfma_reference(qkv16, table, go16, B, H, W, heads, shift, dtype=torch.float64, rnd=None):
    """The reference on the bf16-ROUNDED inputs in the unpadded layout: (output, dqkv, dtable, logits)."""
    M = qkv16.shape[0]
    qd = qkv16.to(dtype).view(M, 3, heads, HP)[..., :30].reshape(M, 3 * heads * 30).requires_grad_(True)
    td = table.to(dtype).requires_grad_(True)
    ref = _attention_reference(qd, td, B, H, W, heads, shift, rnd=rnd)
    rq, rt = torch.autograd.grad(ref, [qd, td], go16.to(dtype).view(M, heads, HP)[..., :30].reshape(M, heads * 30))
    with torch.no_grad():
        logits, _ = attention_logits(qd, td, B, H, W, heads, shift)
    return ref.detach(), rq, rt, logits


def _mfma_run(qkv16, table, go16, B, H, W, heads, shift):
    """Both MFMA kernels on NaN-filled outputs: (out (M, heads, 32), lse (heads, windows, 64), dqkv (M, 3, heads, 32),
    dtable), as float tensors on the host."""
    import _native as N
    M = qkv16.shape[0]
    scale = 30 ** -0.5
    qc, tc, gc = qkv16.cuda(), table.cuda(), go16.cuda()
    out16 = torch.full((M, heads * HP), float("nan"), dtype=torch.bfloat16, device="cuda")
    lse = torch.full((heads, M), float("nan"), dtype=torch.float32, device="cuda")
    N.call("sei_swin_attn_fwd_bf16", qc.data_ptr(), tc.data_ptr(), out16.data_ptr(), lse.data_ptr(), B, H, W, heads, shift,
           scale)
    dqkv16 = torch.full((M, 3 * heads * HP), float("nan"), dtype=torch.bfloat16, device="cuda")
    dtable = torch.zeros_like(tc)
    N.call("sei_swin_attn_bwd_bf16", qc.data_ptr(), tc.data_ptr(), out16.data_ptr(), lse.data_ptr(), gc.data_ptr(),
           dqkv16.data_ptr(), dtable.data_ptr(), B, H, W, heads, shift, scale)
    return (out16.float().cpu().view(M, heads, HP), lse.cpu().view(heads, M // 64, 64),
            dqkv16.float().cpu().view(M, 3, heads, HP), dtable.cpu())


def _lse_reference(logits):
    """(heads, windows in partition order, 64 queries): the rows' log-sum-exp in log2 units (include/sei_hip.h)."""
    return (torch.logsumexp(logits, -1) * math.log2(math.e)).permute(1, 0, 2)


@pytest.mark.parametrize("heads", [1, 2, 3, 6])
@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_mfma_window_attention_geometry_grid(geom, shift, heads):
    """The MFMA kernels on the same extents (one window: three of a workgroup's four waves idle; every window a
    last-row window, so the unmasked fast path of the shifted kernel never runs), with one head (the pair's second
    wave computes a copy / idles), two, three and six: outputs, dqkv and dtable at test_window_attention_mfma_fwd_bwd's
    bars (1e-2 / 2e-2), pad lanes exactly zero, and the stored log-sum-exp EQUAL to the float64 reference's in the
    header's layout and units (1e-5 of max(1, |lse|): float32 scores and one v_exp / v_log each)."""
    B, H, W = geom
    gen = torch.Generator().manual_seed(1000 * H + 10 * W + B + 100 * shift + heads)
    M = B * H * W
    qkv16 = _pad_heads(torch.randn((M, 3, heads, 30), generator=gen), M, 3, heads)
    table = torch.randn((225, heads), generator=gen) * 0.5
    go16 = _pad_heads(torch.randn((M, 1, heads, 30), generator=gen), M, 1, heads)
    ref, rq, rt, logits = _mfma_reference(qkv16, table, go16, B, H, W, heads, shift)
    out, lse, dq, dtable = _mfma_run(qkv16, table, go16, B, H, W, heads, shift)
    lse_ref = _lse_reference(logits)
    lse_err = float(((lse.double() - lse_ref).abs() / lse_ref.abs().clamp(min=1.0)).max())
    errs = relerr(out[..., :30].reshape(M, -1), ref), relerr(dq[..., :30].reshape(M, -1), rq), relerr(dtable, rt)
    print(f"mfma {geom} shift {shift} heads {heads}: out {errs[0]:.2e} dqkv {errs[1]:.2e} dtable {errs[2]:.2e} "
          f"lse {lse_err:.2e}")
    assert bool(torch.isfinite(lse).all()) and lse_err < 1e-5, lse_err
    assert float(out[..., 30:].abs().max()) == 0.0 and float(dq[..., 30:].abs().max()) == 0.0
    assert errs[0] < 1e-2, errs
    assert errs[1] < 2e-2 and errs[2] < 2e-2, errs


def test_mfma_window_attention_refuses_other_shifts():
    """The MFMA mask logic is built for shift 0 / 4: any other shift is an argument error and nothing is written."""
    import _native as N
    B, H, W, heads = 1, 8, 24, 2
    M = B * H * W
    gen = torch.Generator().manual_seed(2)
    qc = _pad_heads(torch.randn((M, 3, heads, 30), generator=gen), M, 3, heads).cuda()
    gc = _pad_heads(torch.randn((M, 1, heads, 30), generator=gen), M, 1, heads).cuda()
    tc = (torch.randn((225, heads), generator=gen) * 0.5).cuda()
    out16 = torch.full((M, heads * HP), float("nan"), dtype=torch.bfloat16, device="cuda")
    lse = torch.full((heads, M), float("nan"), dtype=torch.float32, device="cuda")
    with pytest.raises(N.NativeLibraryError, match="SEI_ERR_BAD_ARG"):
        N.call("sei_swin_attn_fwd_bf16", qc.data_ptr(), tc.data_ptr(), out16.data_ptr(), lse.data_ptr(), B, H, W, heads, 2,
               30 ** -0.5)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out16).all()) and bool(torch.isnan(lse).all())
    dqkv16 = torch.full((M, 3 * heads * HP), float("nan"), dtype=torch.bfloat16, device="cuda")
    dtable = torch.full_like(tc, 3.0)
    lse.zero_()
    out16.zero_()
    with pytest.raises(N.NativeLibraryError, match="SEI_ERR_BAD_ARG"):
        N.call("sei_swin_attn_bwd_bf16", qc.data_ptr(), tc.data_ptr(), out16.data_ptr(), lse.data_ptr(), gc.data_ptr(),
               dqkv16.data_ptr(), dtable.data_ptr(), B, H, W, heads, 2, 30 ** -0.5)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dqkv16).all()) and bool((dtable == 3.0).all())


# ------------------------------------------------------------------------------- large logits and the finite mask
LARGE = [(1, 8, 24), (2, 16, 16)]
LARGE_HEADS = 6


def _large_logit_inputs(B, H, W, heads, hd):
    """q and k scaled for logits (q . k / sqrt(hd)) of standard deviation ~30, a bias table of 20 randn. With ONE common
    scale the masked keys hold 1e-3 of a row's probability in 0.2 % of the rows of masked windows (a masked key has to
    beat the row's best unmasked one by ~93, three standard deviations of that difference), so the keys of one token in
    16 are 8x longer than the others' -- the outlier-norm tokens trained attention layers have -- and the rest shorter,
    the standard deviation over all pairs staying at 30: 14-17 % of the rows then qualify."""
    gen = torch.Generator().manual_seed(100 * H + W + B)
    M = B * H * W
    qkv = torch.randn((M, 3, heads, hd), generator=gen)
    amp = torch.ones(M)
    amp[torch.randperm(M, generator=gen)[:M // 16]] = 8.0
    qkv[:, 0] *= 30.0 ** 0.5
    qkv[:, 1] *= 30.0 ** 0.5 / float((amp ** 2).mean().sqrt()) * amp.view(M, 1, 1)
    table = 20.0 * torch.randn((225, heads), generator=gen)
    go = torch.randn((M, 1, heads, hd), generator=gen)
    return qkv, table, go


def _assert_large_logit_conditions(logits, qk_std, B, H, W, heads):
    """What makes the case a test of the max subtraction and of the FINITE mask, on the float64 reference alone:
    (a) a logit above 90 (expf of it overflows float32); (b) in >= 10 % of the query rows of masked windows the masked
    keys together hold > 1e-3 of the probability (a -inf mask moves those rows by 1e-3 and more)."""
    mask = sp.shift_mask(H, W, 8, 4)
    nW = mask.shape[0]
    masked_keys = (mask != 0).view(1, nW, 1, 64, 64)
    mass = (logits.softmax(-1).view(B, nW, heads, 64, 64) * masked_keys).sum(-1)
    rows = mass[:, (mask != 0).flatten(1).any(1)]
    frac = float((rows > 1e-3).double().mean())
    print(f"large logits {(B, H, W)}: q.k std {qk_std:.1f}, max logit {float(logits.max()):.0f}, rows of masked windows "
          f"with > 1e-3 on masked keys {frac:.3f}, largest such mass {float(rows.max()):.3f}")
    assert 25.0 < qk_std < 35.0
    assert float(logits.max()) > 90.0
    assert frac >= 0.10


def _qk_std(qkv, B, H, W, heads):
    zero = torch.zeros((225, heads), dtype=qkv.dtype)
    return float(attention_logits(qkv, zero, B, H, W, heads, 0)[0].std())


@pytest.mark.parametrize("geom", LARGE, ids=_gid)
def test_f32_window_attention_large_logits_finite_mask(geom):
    """The f32 kernels where the max subtraction and the finiteness of the -100 mask matter (conditions asserted on
    the float64 reference before the launch). Float32 rounding of logits of a few hundred moves the probabilities, so
    the bar is 3x the deviation of THIS reference evaluated in torch float32 on the CPU from its float64 self, floored
    at the geometry grid's 5e-6 / 2e-5; it never looks at the kernel's output.
    Observed reference deviations (float32 CPU vs float64), out / dqkv / dtable:
      (1, 8, 24): 6.5e-6 / 9.7e-6 / 3.4e-6      (2, 16, 16): 6.4e-6 / 8.1e-6 / 5.7e-6"""
    B, H, W = geom
    heads, hd = LARGE_HEADS, 30
    M = B * H * W
    q4, table, go4 = _large_logit_inputs(B, H, W, heads, hd)
    qkv, go = q4.reshape(M, -1), go4.reshape(M, -1)
    with torch.no_grad():
        logits, _ = attention_logits(qkv.double(), table.double(), B, H, W, heads, 4)
    _assert_large_logit_conditions(logits, _qk_std(qkv.double(), B, H, W, heads), B, H, W, heads)
    q32, t32 = qkv.clone().requires_grad_(True), table.clone().requires_grad_(True)
    r32 = _attention_reference(q32, t32, B, H, W, heads, 4)
    rq32, rt32 = torch.autograd.grad(r32, [q32, t32], go)
    (ref, rq, rt), (out, dqkv, dtable) = _f32_case(B, H, W, heads, hd, 4, qkv, table, go)
    dev = relerr(r32, ref), relerr(rq32, rq), relerr(rt32, rt)
    bars = max(5e-6, 3 * dev[0]), max(2e-5, 3 * dev[1]), max(2e-5, 3 * dev[2])
    errs = relerr(out, ref), relerr(dqkv, rq), relerr(dtable, rt)
    print(f"f32 large logits {geom}: float32 reference deviates {dev[0]:.2e} / {dev[1]:.2e} / {dev[2]:.2e}; kernel "
          f"{errs[0]:.2e} / {errs[1]:.2e} / {errs[2]:.2e}")
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dqkv).all())
    assert errs[0] < bars[0], (errs, bars)
    assert errs[1] < bars[1] and errs[2] < bars[2], (errs, bars)


@pytest.mark.parametrize("geom", LARGE, ids=_gid)
def test_mfma_window_attention_large_logits_finite_mask(geom):
    """The MFMA kernels on the same inputs rounded to bf16 (conditions asserted on the float64 reference of the ROUNDED
    inputs): the forward's max subtraction, the backward's `-100 / scale` on top of `bias / scale` and its
    exp2(c S - lse) with the folded scale. Bar: 3x the deviation from float64 of the float32 reference with its
    probabilities and its result rounded to bf16 (autograd rounds the gradients at the same two places), floored at the
    geometry grid's 1e-2 / 2e-2. The stored log-sum-exp is held to the float64 one as in the grid.
    Observed reference deviations (float32 + bf16 roundings vs float64), out / dqkv / dtable:
      (1, 8, 24): 3.2e-3 / 1.7e-3 / 1.6e-3      (2, 16, 16): 3.3e-3 / 1.9e-3 / 2.1e-3"""
    B, H, W = geom
    heads = LARGE_HEADS
    M = B * H * W
    q4, table, go4 = _large_logit_inputs(B, H, W, heads, 30)
    qkv16, go16 = _pad_heads(q4, M, 3, heads), _pad_heads(go4, M, 1, heads)
    ref, rq, rt, logits = _mfma_reference(qkv16, table, go16, B, H, W, heads, 4)
    qr = qkv16.double().view(M, 3, heads, HP)[..., :30].reshape(M, -1)
    _assert_large_logit_conditions(logits, _qk_std(qr, B, H, W, heads), B, H, W, heads)
    r32, rq32, rt32, _ = _mfma_reference(qkv16, table, go16, B, H, W, heads, 4, dtype=torch.float32,
                                         rnd=lambda t: t.bfloat16().float())
    dev = relerr(r32, ref), relerr(rq32, rq), relerr(rt32, rt)
    bars = max(1e-2, 3 * dev[0]), max(2e-2, 3 * dev[1]), max(2e-2, 3 * dev[2])
    out, lse, dq, dtable = _mfma_run(qkv16, table, go16, B, H, W, heads, 4)
    lse_ref = _lse_reference(logits)
    lse_err = float(((lse.double() - lse_ref).abs() / lse_ref.abs().clamp(min=1.0)).max())
    errs = relerr(out[..., :30].reshape(M, -1), ref), relerr(dq[..., :30].reshape(M, -1), rq), relerr(dtable, rt)
    print(f"mfma large logits {geom}: rounded float32 reference deviates {dev[0]:.2e} / {dev[1]:.2e} / {dev[2]:.2e}; "
          f"kernel {errs[0]:.2e} / {errs[1]:.2e} / {errs[2]:.2e}, lse {lse_err:.2e}")
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dq).all())
    assert float(out[..., 30:].abs().max()) == 0.0 and float(dq[..., 30:].abs().max()) == 0.0
    assert lse_err < 1e-5, lse_err
    assert errs[0] < bars[0], (errs, bars)
    assert errs[1] < bars[1] and errs[2] < bars[2], (errs, bars)


# ---------------------------------------------------------------------------------------------- dtable: += , not =
def test_f32_bias_table_gradient_is_added():
    """include/sei_hip.h: `dtable (+=, float atomics)`. models/_swin_ops.py hands the kernel `grad_of(table)`, the
    parameter's slice of the flat gradient bucket, which already holds the step's other model calls' share."""
    B, H, W, heads, hd, shift = 2, 8, 16, 2, 16, 4
    from models import _swin_ops as S
    gen = torch.Generator().manual_seed(21)
    qkv = torch.randn((B * H * W, 3 * heads * hd), generator=gen)
    table = torch.randn((225, heads), generator=gen) * 0.5
    go = torch.randn((B * H * W, heads * hd), generator=gen)
    before = torch.randn((225, heads), generator=gen)
    qd, td = qkv.double().requires_grad_(True), table.double().requires_grad_(True)
    (rt,) = torch.autograd.grad(_attention_reference(qd, td, B, H, W, heads, shift), [td], go.double())
    dtable = before.cuda()
    S.window_attention_bwd(qkv.cuda(), table.cuda(), go.cuda(), dtable, B, H, W, heads, shift)
    assert relerr(dtable.cpu().double() - before.double(), rt) < 2e-5
    S.window_attention_bwd(qkv.cuda(), table.cuda(), go.cuda(), dtable, B, H, W, heads, shift)
    assert relerr(dtable.cpu().double() - before.double(), 2 * rt) < 2e-5


def test_mfma_bias_table_gradient_is_added():
    """include/sei_hip.h: `dtable float (+=)`. models/_swin_ops16.py hands the kernel `grad_of(table)` in every
    block's backward, and a step's model calls follow each other into the same bucket."""
    import _native as N
    B, H, W, heads, shift = 2, 8, 16, 3, 4
    M = B * H * W
    gen = torch.Generator().manual_seed(22)
    qkv16 = _pad_heads(torch.randn((M, 3, heads, 30), generator=gen), M, 3, heads)
    table = torch.randn((225, heads), generator=gen) * 0.5
    go16 = _pad_heads(torch.randn((M, 1, heads, 30), generator=gen), M, 1, heads)
    before = torch.randn((225, heads), generator=gen)
    _, _, rt, _ = _mfma_reference(qkv16, table, go16, B, H, W, heads, shift)
    scale = 30 ** -0.5
    qc, tc, gc = qkv16.cuda(), table.cuda(), go16.cuda()
    out16 = torch.empty((M, heads * HP), dtype=torch.bfloat16, device="cuda")
    lse = torch.empty((heads, M), dtype=torch.float32, device="cuda")
    N.call("sei_swin_attn_fwd_bf16", qc.data_ptr(), tc.data_ptr(), out16.data_ptr(), lse.data_ptr(), B, H, W, heads, shift,
           scale)
    dqkv16 = torch.empty((M, 3 * heads * HP), dtype=torch.bfloat16, device="cuda")
    dtable = before.cuda()
    for times in (1, 2):
        N.call("sei_swin_attn_bwd_bf16", qc.data_ptr(), tc.data_ptr(), out16.data_ptr(), lse.data_ptr(), gc.data_ptr(),
               dqkv16.data_ptr(), dtable.data_ptr(), B, H, W, heads, shift, scale)
        assert relerr(dtable.cpu().double() - before.double(), times * rt) < 2e-2


# ---------------------------------------------------------------------------------------------- the model, thin images
THIN = [(1, 3, 8, 40), (1, 3, 5, 21)]


def _thin_model(seed):
    from models.swinir import SwinIR
    torch.manual_seed(seed)
    model = SwinIR(upscale=1, upsampler=None, depths=(2, 2), num_heads=(6, 6))
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():                               # make every parameter matter (LayerNorm / bias defaults are 1 / 0)
        for k, v in model.named_parameters():
            if k.endswith("bias") or "norm" in k:
                v.add_(0.1 * torch.randn(v.shape, generator=gen))
    return model, gen


@pytest.mark.parametrize("shape", THIN, ids=_gid)
def test_swinir_on_a_thin_image_vs_oracle(shape):
    """Deblurring SwinIR (two depth-2 groups, eval mode, f32) on an 8 x 40 image and on a 5 x 21 one that the forward
    reflect-pads to 8 x 24: the shifted blocks run on ONE window row, the mask being that of the actual extent with the
    shift kept, as the published network recomputes it. Against oracle/swinir_path.py at
    test_swinir_model_vs_oracle's bars (1e-4 forward, 1e-3 every parameter gradient)."""
    model, gen = _thin_model(3)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items() if v.dtype.is_floating_point
          and "attn_mask" not in k}
    model = model.cuda().eval()
    x = torch.rand(shape, generator=gen)
    go = torch.randn(shape, generator=gen)
    ref = sp.swinir_forward(sd, x, upscale=1, drop_masks=None, depths=(2, 2))
    ref.backward(go)
    model.zero_grad_flat()
    out = model(x.cuda(), drop_masks=None)
    assert out.shape == ref.shape == shape
    assert relerr(out, ref) < 1e-4, relerr(out, ref)
    out.backward(go.cuda())
    worst = max((relerr(p.grad, sd[k].grad), k) for k, p in model.named_parameters())
    print(f"thin image {shape}: out {relerr(out, ref):.2e}, worst gradient {worst[0]:.2e} ({worst[1]})")
    assert worst[0] < 1e-3, worst


@pytest.mark.parametrize("shape", THIN, ids=_gid)
def test_swinir_bf16_path_on_a_thin_image_tracks_f32(shape):
    """The same network in throughput mode (MFMA window attention on one window row) against its f32 mode, at
    test_swinir_bf16_path_tracks_f32's bars: restored image 3e-2, every parameter gradient's cosine > 0.98 and norm
    within a factor 2."""
    from models import _ops
    model, gen = _thin_model(6)
    model = model.cuda().eval()
    x = torch.rand(shape, generator=gen).cuda()
    go = torch.randn(shape, generator=gen).cuda()
    outs = {}
    for mode in ("f32", "bf16"):
        prev = _ops.set_compute_dtype(mode)
        try:
            model.zero_grad_flat()
            out = model(x, drop_masks=None)
            out.backward(go)
            torch.cuda.synchronize()
            outs[mode] = (out.detach().clone(), model.flat_grads.clone())
        finally:
            _ops.set_compute_dtype(prev)
    assert relerr(outs["bf16"][0], outs["f32"][0]) < 3e-2, relerr(outs["bf16"][0], outs["f32"][0])
    base = model.flat_params.data_ptr()
    worst = (1.0, "")
    for k, p in model.named_parameters():
        off = (p.data_ptr() - base) // 4
        a, b = outs["bf16"][1][off:off + p.numel()].double(), outs["f32"][1][off:off + p.numel()].double()
        assert float(b.norm()) > 0.0, k
        cos = float(a @ b / (a.norm() * b.norm() + 1e-300))
        worst = min(worst, (cos, k))
        assert 0.5 < float(a.norm() / (b.norm() + 1e-300)) < 2.0, (k, float(a.norm()), float(b.norm()))
    print(f"thin image {shape}: bf16 vs f32 out {relerr(outs['bf16'][0], outs['f32'][0]):.2e}, worst cosine "
          f"{worst[0]:.4f} ({worst[1]})")
    assert worst[0] > 0.98, worst
