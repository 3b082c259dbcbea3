"""The SwinIR streaming kernels between the GEMMs (csrc/swin_bf16_kernels.hip, csrc/swin_kernels.hip), one by one against
tests/streaming_ref.py: sei_ln_fwd_bf16_pad, sei_ln_bwd_pad, sei_cast_pad_bf16, sei_pad_nhwc_bf16[_ones], sei_pack,
sei_unpack_add, sei_pad_nhwc, sei_unpad_nhwc and sei_rowscale, at the channel counts where the `live` lane mask, the ones
lane and the zero padding differ, and at the row / item counts where the grid-stride loops take a second turn.

Bars (streaming_ref.py states them): exact = bit for bit against the same float32 operation on the CPU; float32 =
max(5e-6, 3 * ref32) of the float64 reference (2e-5 for column sums and LayerNorm parameter gradients); bf16 =
2^-8 |ref64| + e32 per element. Every output lies between two sentinel margins of its own allocation and is prefilled with
the sentinel, strides gaps and input tails hold NaN.

Measured on one MI355X (largest over the cases of a family; ref32 is the float32 CPU chain, bar the resulting bound):
    family                            ref32     bar       HIP deviation
    ln_fwd_bf16_pad mean              1.7e-7    5.0e-6    1.9e-7
    ln_fwd_bf16_pad rstd              1.6e-7    5.0e-6    1.4e-7
    ln_bwd_pad gx                     8.1e-7    5.0e-6    7.6e-7
    ln_bwd_pad ggamma                 4.1e-7    2.0e-5    3.0e-7
    ln_bwd_pad gbeta                  2.2e-7    2.0e-5    2.3e-7
    ln_bwd_pad partial rows, ggamma   4.3e-7    2.0e-5    1.6e-7
    ln_bwd_pad partial rows, gbeta    2.4e-7    2.0e-5    8.9e-8
    cast_pad_bf16 colsum              2.1e-7    2.0e-5    3.2e-7
    unpad_nhwc act + res              4.8e-8    5.0e-6    4.8e-8
    ln_fwd_bf16_pad y (bf16 bar): e32 between 1.7e-7 (no special rows) and 1.4e-4; the worst |got - ref64| - 2^-8 |ref64|
    was 5.9e-6 where e32 was 4.0e-5, at most 0.15 of e32 in any case.
So the floors, not measured bars, are what every family here is held to.
Everything else in this module is held bit for bit.
"""
import pytest
import torch
import torch.nn.functional as F

import streaming_ref as R

pytestmark = pytest.mark.gpu
EPS = 1e-5
CAP_ITEMS = 4096 * 256                      # items of one sweep of the capped streaming grids
GEOMETRIES = [(1, 1, 1, 0), (2, 3, 5, 7), (1, 8, 8, 10), (3, 2, 9, 3), (2, 126, 126, 129)]       # (B, H, W, guard)


def native():
    import _native
    return _native


def refused(name, *args):
    N = native()
    with pytest.raises(N.NativeLibraryError):
        N.call(name, *args)
    torch.cuda.synchronize()


def f32_guard(shape):
    return R.Guarded(shape)


def bf16_guard(shape):
    return R.Guarded(shape, dtype=torch.bfloat16)


# ------------------------------------------------------------------------------------------------ sei_ln_fwd_bf16_pad
LN_FWD = [(180, 192, 1), (180, 192, 0), (4, 8, 1), (4, 4, 0), (60, 64, 1), (64, 64, 0), (252, 256, 1), (256, 256, 0),
          (180, 256, 1)]
LN_C = sorted({c for c, _, _ in LN_FWD})


@pytest.mark.parametrize("rows", [1, 3, 5, 4099, 16390])
@pytest.mark.parametrize("C,ldy,ones", LN_FWD)
def test_ln_fwd_bf16_pad(C, ldy, ones, rows):
    """(252, 256, 1): the last lane is the ones lane; (256, 256, 0): every lane live, no pad; (180, 256, 1): all-zero pad
    lanes behind the ones lane; 16390 rows > 4 * 4096: a second turn of the row loop, which also takes the constant row
    (rstd = 1 / sqrt(eps), y = beta) and the row of mean 100."""
    N = native()
    x, gamma, beta, _, _ = R.ln_inputs(rows, C, 1000 * C + ldy + rows, special_rows=True)
    y64, m64, r64 = R.ln_fwd(x, gamma, beta, EPS, torch.float64)
    y32, m32, r32 = R.ln_fwd(x, gamma, beta, EPS, torch.float32)
    y, mean, rstd = bf16_guard((rows, ldy)), f32_guard(rows), f32_guard(rows)
    xd, gd, bd = R.nan_tailed(x), R.nan_tailed(gamma), R.nan_tailed(beta)
    N.call("sei_ln_fwd_bf16_pad", xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.ptr(), mean.ptr(), rstd.ptr(), rows, C, ldy,
           EPS, ones)
    torch.cuda.synchronize()
    assert y.intact() and mean.intact() and rstd.intact()
    got = y.view.cpu()
    R.hold_bf16(f"ln_fwd y C={C} rows={rows}", got[:, :C], y64, y32)
    # (the row of mean 100 and the constant row's rstd = 316 on their own: they would set the max-norm for every row)
    for lo, hi in ((0, rows - 2), (rows - 2, rows - 1), (rows - 1, rows)) if rows >= 3 else ((0, rows),):
        R.hold32(f"ln_fwd mean C={C} rows {lo}..{hi - 1} of {rows}", mean.view[lo:hi], m64[lo:hi], m32[lo:hi])
        R.hold32(f"ln_fwd rstd C={C} rows {lo}..{hi - 1} of {rows}", rstd.view[lo:hi], r64[lo:hi], r32[lo:hi])
    want_pad = torch.zeros((rows, ldy - C), dtype=torch.bfloat16)
    if ones:
        want_pad[:, 0] = 1.0
    assert R.same_bits(got[:, C:], want_pad)
    if rows >= 3:                                               # the constant row: y = bf16(beta), exactly
        assert R.same_bits(got[rows - 1, :C], beta.bfloat16())


def test_ln_fwd_bf16_pad_refusals():
    x, g, y, s = (torch.zeros(4 * 272, device="cuda"), torch.zeros(272, device="cuda"),
                  torch.zeros(4 * 272, device="cuda", dtype=torch.bfloat16), torch.zeros(8, device="cuda"))
    args = lambda C, ldy, ones: (x.data_ptr(), g.data_ptr(), g.data_ptr(), y.data_ptr(), s.data_ptr(), s.data_ptr(), 4, C,
                                 ldy, EPS, ones)
    refused("sei_ln_fwd_bf16_pad", *args(180, 180, 1))           # no padding column for the ones
    refused("sei_ln_fwd_bf16_pad", *args(6, 8, 0))               # C % 4 != 0
    refused("sei_ln_fwd_bf16_pad", *args(260, 264, 0))           # C > 256
    native().call("sei_ln_fwd_bf16_pad", *args(180, 192, 1))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ sei_ln_bwd_pad
@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("gap", [0, 12])
@pytest.mark.parametrize("C", LN_C)
def test_ln_bwd_pad(C, gap, with_res):
    """gy with row stride ldg = C + gap (C = 180: 192) and NaN in the gap; 4099 + 4096 rows > 4 * 1024 workgroups: a wave
    accumulates more than one row. gx, ggamma, gbeta (on top of random start values) and the partial rows left in `work`,
    summed in float64, against torch.autograd.grad of F.layer_norm in float64."""
    N = native()
    ldg = C + gap
    need = N.lib().sei_swin_partials_floats(C)
    assert need == 1024 * 2 * C
    for rows in (1, 3, 50, 4100, 4099 + 4096):
        x, gamma, beta, gy, res = R.ln_inputs(rows, C, 77 * C + gap + rows)
        res = res if with_res else None
        _, mean, rstd = R.ln_fwd(x, gamma, beta, EPS, torch.float32)          # the float32 statistics the kernel is handed
        gx64, gg64, gb64 = R.ln_bwd_autograd(x, gamma, gy, EPS, res)
        gx32, gg32, gb32 = R.ln_bwd(x, gamma, mean, rstd, gy, torch.float32, res)
        gen = torch.Generator().manual_seed(rows)
        gg0, gb0 = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
        gy_wide = torch.full((rows, ldg), float("nan"))
        gy_wide[:, :C] = gy
        groups = min((rows + 3) // 4, 1024)
        gx, work = f32_guard((rows, C)), f32_guard(need)
        gg, gb = f32_guard(C), f32_guard(C)
        gg.view.copy_(gg0); gb.view.copy_(gb0)
        dev = [R.nan_tailed(t) for t in (x, gamma, mean, rstd, gy_wide)]
        resd = R.nan_tailed(res) if with_res else None
        N.call("sei_ln_bwd_pad", *(t.data_ptr() for t in dev), N.ptr(resd), gx.ptr(), gg.ptr(), gb.ptr(), rows, C, ldg,
               work.ptr(), need)
        torch.cuda.synchronize()
        assert gx.intact() and work.intact() and gg.intact() and gb.intact()
        label = f"ln_bwd C={C} ldg={ldg} rows={rows} res={int(with_res)}"
        R.hold32(label + " gx", gx.view, gx64, gx32)
        R.hold32(label + " ggamma", gg.view, gg0.double() + gg64, gg0 + gg32, R.REDUCTION_FLOOR)
        R.hold32(label + " gbeta", gb.view, gb0.double() + gb64, gb0 + gb32, R.REDUCTION_FLOOR)
        w = work.view.cpu()
        assert bool((w[groups * 2 * C:] == R.SENTINEL).all())                   # these are all the partial rows it wrote
        part = w[:groups * 2 * C].view(groups, 2 * C).double().sum(0)
        R.hold32(label + " partial ggamma", part[:C], gg64, gg32, R.REDUCTION_FLOOR)
        R.hold32(label + " partial gbeta", part[C:], gb64, gb32, R.REDUCTION_FLOOR)


# ------------------------------------------------------------------------------------------------ sei_cast_pad_bf16
@pytest.mark.parametrize("with_colsum", [True, False], ids=["colsum", "nocolsum"])
@pytest.mark.parametrize("with_scale", [True, False], ids=["scale", "noscale"])
@pytest.mark.parametrize("C,ldy", [(180, 192), (180, 180), (4, 8), (256, 256), (60, 256)])
def test_cast_pad_bf16(C, ldy, with_scale, with_colsum):
    """Rows bit for bit against (x * s[:, None]).bfloat16() (the product is rounded to float32 before the conversion, so
    a contraction of the column sums' multiply-add cannot change them), pads exact zeros, column sums on top of random
    start values against float64 sums of the float32-scaled rows. 8200 rows > 4 * 1024 workgroups."""
    N = native()
    need = N.lib().sei_swin_partials_floats(C)
    for rows in (1, 3, 300, 4100, 8200):
        gen = torch.Generator().manual_seed(13 * C + ldy + rows)
        x = torch.randn((rows, C), generator=gen)
        scale = torch.rand(rows, generator=gen) * 1.25 if with_scale else None
        if with_scale and rows >= 3:
            scale[1] = 0.0                                                  # a dropped row (stochastic depth)
        cs0 = torch.randn(C, generator=gen)
        v, v16 = R.scaled_cast(x, scale)
        y, cs, work = bf16_guard((rows, ldy)), f32_guard(C), f32_guard(need)
        cs.view.copy_(cs0)
        xd = R.nan_tailed(x)
        sd = R.nan_tailed(scale) if with_scale else None
        N.call("sei_cast_pad_bf16", xd.data_ptr(), N.ptr(sd), y.ptr(), cs.ptr() if with_colsum else None, rows, C, ldy,
               work.ptr() if with_colsum else None, need if with_colsum else 0)
        torch.cuda.synchronize()
        assert y.intact() and cs.intact() and work.intact()
        got = y.view.cpu()
        assert R.same_bits(got[:, :C], v16), (rows, "rows")
        assert R.same_bits(got[:, C:], torch.zeros((rows, ldy - C), dtype=torch.bfloat16)), (rows, "pad")
        if with_colsum:
            R.hold32(f"cast_pad colsum C={C} rows={rows} scale={int(with_scale)}", cs.view, cs0.double() + v.double().sum(0),
                     cs0 + v.sum(0), R.REDUCTION_FLOOR)
        else:
            assert R.same_bits(cs.view, cs0) and bool((work.view == R.SENTINEL).all())


# ------------------------------------------------------------------------------------------------ sei_pad_nhwc_bf16[_ones]
# (4, 126, 126, 60, 64, 129): 65794 rows of 16 ushort4 = 1,052,704 items, past 4096 x 256 (the 2-image case has 528,416)
@pytest.mark.parametrize("B,H,W,C,Cp,guard", [(1, 1, 1, 4, 8, 0), (2, 3, 5, 60, 64, 7), (1, 8, 8, 180, 192, 10),
                                              (3, 2, 9, 64, 64, 3), (2, 126, 126, 60, 64, 129),
                                              (4, 126, 126, 60, 64, 129)])
def test_pad_nhwc_bf16(B, H, W, C, Cp, guard):
    """Against F.pad of the bf16 copy; with ones_col channel C is 1.0 in every row, border and guard rows included."""
    N = native()
    x = torch.randn((B, H, W, C), generator=torch.Generator().manual_seed(B + H + C + guard))
    want = F.pad(F.pad(x.bfloat16(), (0, Cp - C, 1, 1, 1, 1)).view(-1, Cp), (0, 0, guard, guard))
    assert R.same_bits(want, R.padded_grid(x.bfloat16(), guard, Cp))
    rows = want.shape[0]
    if B == 4:
        assert rows * (Cp // 4) > CAP_ITEMS
    xd = R.nan_tailed(x)
    for ones in ((0, 1) if Cp > C else (0,)):
        ref = want.clone()
        if ones:
            ref[:, C] = 1.0
        out = bf16_guard((rows, Cp))
        N.call("sei_pad_nhwc_bf16_ones", xd.data_ptr(), out.ptr(), B, H, W, C, Cp, guard, ones)
        torch.cuda.synchronize()
        assert out.intact() and R.same_bits(out.view, ref), ones
    out = bf16_guard((rows, Cp))
    N.call("sei_pad_nhwc_bf16", xd.data_ptr(), out.ptr(), B, H, W, C, Cp, guard)
    torch.cuda.synchronize()
    assert out.intact() and R.same_bits(out.view, want)
    if Cp == C:
        refused("sei_pad_nhwc_bf16_ones", xd.data_ptr(), out.ptr(), B, H, W, C, Cp, guard, 1)


# ------------------------------------------------------------------------------------------------ sei_pack, sei_unpack_add
@pytest.mark.parametrize("to_bf16", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 257, 1_048_576 + 300])
def test_pack(n, to_bf16):
    """dst[i] = src[map[i]], zeros in the -1 holes; 1,048,876 elements > 4096 x 256: the loop's second turn."""
    N = native()
    n_src = n + 37
    m = R.index_map(n, n_src, n)
    if n >= 255:
        assert 0.05 * n < int((m < 0).sum()) < 0.15 * n
    src = torch.randn(n_src, generator=torch.Generator().manual_seed(n + 1))
    want = R.pack_ref(src, m)
    out = bf16_guard(n) if to_bf16 else f32_guard(n)
    srcd, md = R.nan_tailed(src), R.nan_tailed(m)
    N.call("sei_pack", srcd.data_ptr(), md.data_ptr(), out.ptr(), n, to_bf16)
    torch.cuda.synchronize()
    assert out.intact() and R.same_bits(out.view, want.bfloat16() if to_bf16 else want)


@pytest.mark.parametrize("n", [1, 255, 257, 1_048_576 + 300])
def test_unpack_add(n):
    """dst[map[i]] += src[i] on random destinations, every target at most once; untouched elements keep their bits."""
    N = native()
    n_dst = n + 37
    m = R.index_map(n, n_dst, n + 5)
    gen = torch.Generator().manual_seed(n + 2)
    src, dst0 = torch.randn(n, generator=gen), torch.randn(n_dst, generator=gen)
    dst = f32_guard(n_dst)
    dst.view.copy_(dst0)
    srcd, md = R.nan_tailed(src), R.nan_tailed(m)
    N.call("sei_unpack_add", srcd.data_ptr(), md.data_ptr(), dst.ptr(), n)
    torch.cuda.synchronize()
    assert dst.intact() and R.same_bits(dst.view, R.unpack_add_ref(src, m, dst0))


# ------------------------------------------------------------------------------------------------ sei_pad_nhwc
@pytest.mark.parametrize("C", [4, 60, 180])
@pytest.mark.parametrize("B,H,W,guard", GEOMETRIES)
def test_pad_nhwc(B, H, W, guard, C):
    """Zero border and guards, exact interior; (2, 126, 126, 129) x 180 channels is 1,486,170 float4 items > 4096 x 256."""
    N = native()
    x = torch.randn((B, H, W, C), generator=torch.Generator().manual_seed(B + H + C + guard))
    want = R.padded_grid(x, guard)
    if B * H * W * C == 2 * 126 * 126 * 180:
        assert want.numel() // 4 > CAP_ITEMS
    out = f32_guard(want.shape)
    xd = R.nan_tailed(x)
    N.call("sei_pad_nhwc", xd.data_ptr(), out.ptr(), B, H, W, C, guard)
    torch.cuda.synchronize()
    assert out.intact() and R.same_bits(out.view, want)


# ------------------------------------------------------------------------------------------------ sei_unpad_nhwc
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("B,H,W,guard,C", [(1, 1, 1, 0, 4), (2, 3, 5, 7, 60), (3, 2, 9, 3, 180), (1, 8, 8, 10, 4),
                                           (2, 126, 126, 129, 180)])
def test_unpad_nhwc(B, H, W, guard, C, act, with_res):
    """The interior of a padded grid whose border and guard rows hold garbage; negative, 0.0, -0.0 and positive values for
    the LeakyReLU; act alone and res alone are one float32 operation (bit for bit), act + res may contract 0.01 v + r
    into one FMA and takes the float32 bar. (2, 126, 126) x 180 channels: 1,428,840 float4 items > 4096 x 256."""
    N = native()
    gen = torch.Generator().manual_seed(B + H + W + C + act)
    x = torch.randn((B, H, W, C), generator=gen)
    flat = x.view(-1)
    k = min(4, flat.numel())
    flat[:k] = torch.tensor([-1.5, 0.0, -0.0, 2.5])[:k]
    res = torch.randn((B, H, W, C), generator=gen) if with_res else None
    inside = R.padded_grid(torch.ones_like(x), guard) != 0
    xp = torch.where(inside, R.padded_grid(x, guard), torch.full(inside.shape, 1e4) + torch.randn(inside.shape, generator=gen))
    xpd = R.nan_tailed(xp)
    out = f32_guard((B, H, W, C))
    resd = R.nan_tailed(res) if with_res else None
    N.call("sei_unpad_nhwc", xpd[guard:].data_ptr(), N.ptr(resd), out.ptr(), B, H, W, C, act)
    torch.cuda.synchronize()
    assert out.intact()
    v32 = R.leaky(x) if act else x
    if not (act and with_res):
        assert R.same_bits(out.view, v32 + res if with_res else v32)
    else:
        v64 = torch.where(x > 0, x.double(), x.double() * float(torch.tensor(0.01)))      # the float32 slope, as handed
        R.hold32(f"unpad act + res {B}x{H}x{W}x{C}", out.view, v64 + res.double(), v32 + res)


# ------------------------------------------------------------------------------------------------ sei_rowscale
@pytest.mark.parametrize("mode", ["scale", "gate", "both"])
@pytest.mark.parametrize("M,Nn", [(1, 4), (7, 180), (5000, 180), (24000, 180)])
def test_rowscale(M, Nn, mode):
    """(x * s) * (gate > 0 ? 1 : 0.01) in that order, every step one float32 multiply; gates hold 0.0 and -0.0 (not > 0:
    the 0.01 branch); 24000 x 180 is 1,080,000 float4 items > 4096 x 256."""
    N = native()
    gen = torch.Generator().manual_seed(M + Nn)
    x, s, gate = torch.randn((M, Nn), generator=gen), torch.rand(M, generator=gen) * 1.25, torch.randn((M, Nn), generator=gen)
    gate.view(-1)[:4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30])
    if M == 24000:
        assert M * Nn // 4 > CAP_ITEMS
    want = x
    if mode != "gate":
        want = want * s[:, None]
    if mode != "scale":
        want = want * R.leaky_gate(gate)
    out = f32_guard((M, Nn))
    xd, sd, gated = R.nan_tailed(x), R.nan_tailed(s), R.nan_tailed(gate)
    N.call("sei_rowscale", xd.data_ptr(), sd.data_ptr() if mode != "gate" else None,
           gated.data_ptr() if mode != "scale" else None, out.ptr(), M, Nn)
    torch.cuda.synchronize()
    assert out.intact() and R.same_bits(out.view, want)


def test_rowscale_refuses_no_factor():
    x = torch.zeros((4, 8), device="cuda")
    refused("sei_rowscale", x.data_ptr(), None, None, torch.empty_like(x).data_ptr(), 4, 8)
