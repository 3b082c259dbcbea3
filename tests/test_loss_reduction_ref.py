"""tests/loss_reduction_ref.py on the CPU: the references that tests/test_loss_reductions_gpu.py holds the loss reductions
and the column sums to are anchored first -- SURE to the oracle's sure_loss and its float64 autograd on a square cropped
and an uncropped case, the squared error to F.mse_loss and autograd, the luma to metrics.luma and the oracle's psnr_y,
the column sums to (w[:, None] * X).sum(0) -- and `ref32` of every family is measured on every case the GPU module draws:
below a third of its floor, so the floor is the bar (loss_reduction_ref.MEASURED_REF32 records the printed values)."""
import pytest
import torch
import torch.nn.functional as F

import loss_reduction_ref as L
import streaming_ref as R
from oracle import torch_path as tp

F64 = torch.float64


# ---------------------------------------------------------------------------------------------- anchors
@pytest.mark.parametrize("case,cropped", [((3, 48, 48, 6, 6), True), ((3, 48, 48, 0, 6), False)])
@pytest.mark.parametrize("border_b", [False, True])
def test_sure_reference_is_the_oracles_sure_loss(case, cropped, border_b):
    """Value and both gradients against oracle/torch_path.py's sure_loss in float64 (A = identity, x_net = y1, the model
    returns y2), with the scalars as Python floats on both sides. With b nonzero on the border the oracle is handed b's
    interior, as its own draw would be: the reference's masks must make the same cut."""
    planes, H, W, md, mm = case
    y, y1, y2, b = L.sure_inputs(*case, border_b)
    c_mse, c_div, cst = L.sure_constants(*case)
    ref = L.sure(y, y1, y2, b, md, mm, L.TAU, c_mse, c_div, cst, F64, rounded=False)
    img = lambda t: t.double()[:, None]                                              # (B, 1, H, W)
    x_net, out2 = img(y1).requires_grad_(True), img(y2).requires_grad_(True)
    b_in = img(b)[:, :, md:H - md, md:W - md]
    want = tp.sure_loss(img(y), x_net, lambda t: t, lambda t: out2, L.SIGMA, margin=mm, tau=L.TAU, cropped_div=cropped,
                        b=b_in)
    g1, g2 = torch.autograd.grad(want, [x_net, out2])
    want = want.detach()
    assert abs(float(ref["loss"]) - float(want)) <= 1e-12 * float(ref["loss_scale"])
    assert R.relerr(ref["g1"], g1[:, 0]) < 1e-12 and R.relerr(ref["g2"], g2[:, 0]) < 1e-12
    # the float32-rounded scalars move it by a few 2^-24, and no further
    rounded = L.sure(y, y1, y2, b, md, mm, L.TAU, c_mse, c_div, cst, F64)
    assert 0 < abs(float(rounded["loss"]) - float(want)) <= 4 * 2.0 ** -24 * float(ref["loss_scale"])


@pytest.mark.parametrize("planes,H,W,md,mm,border_b", L.SURE_CASES)
def test_sure_reference_counts_and_zeros(planes, H, W, md, mm, border_b):
    """The interiors have the sizes losses/sure.py divides by, the gradients vanish outside them (+0.0 in float32, as the
    kernel's `0.f`), b is as border_b says, and the sums are those of the slices."""
    (y, y1, y2, b), _, r64, r32 = L.sure_case(planes, H, W, md, mm, border_b)
    in_d, in_m = L.interior(H, W, md), L.interior(H, W, mm)
    assert int(in_d.sum()) == (H - 2 * md) * (W - 2 * md) >= 1 and int(in_m.sum()) == (H - 2 * mm) * (W - 2 * mm) >= 1
    assert bool((b[:, in_d] != 0).all()) and bool((b[:, ~in_d] != 0).all()) == (border_b or md == 0)
    for r in (r64, r32):
        assert bool((r["g2"][:, in_d] != 0).all()) and bool((r["g1"][:, in_d | in_m] != 0).all())
    zeros = torch.zeros((planes, int((~in_d).sum())))
    assert R.same_bits(r32["g2"][:, ~in_d], zeros)
    assert R.same_bits(r32["g1"][:, ~(in_d | in_m)], torch.zeros((planes, int((~(in_d | in_m)).sum()))))
    yd, y1d, y2d, bd = (t.double() for t in (y, y1, y2, b))
    tau = float(L.f32(L.TAU))
    cut = lambda t, m: t[:, m:H - m, m:W - m]
    assert float(r64["div"]) == pytest.approx(float((cut(bd, md) * cut(y2d - y1d, md) / tau).sum()), rel=1e-9, abs=1e-12)
    assert float(r64["mse"]) == pytest.approx(float(cut(y1d - yd, mm).pow(2).sum()), rel=1e-12)
    assert float(r64["abs_div"]) >= abs(float(r64["div"]))


@pytest.mark.parametrize("kind", L.MSE_SCALES)
@pytest.mark.parametrize("n", [3, 1025])
def test_mse_reference_is_f_mse_loss(n, kind):
    a, b = L.mse_inputs(n)
    gs, vs = L.mse_scales(kind, n)
    ref = L.mse(a, b, gs, vs, F64, rounded=False)
    ar = a.double().requires_grad_(True)
    w = vs * n
    want = w * F.mse_loss(ar, b.double())
    (ga,) = torch.autograd.grad(want, ar)
    want = want.detach()
    assert float(ref["value"]) == pytest.approx(float(want), rel=1e-12)
    assert float(ref["sum"]) == pytest.approx(float(F.mse_loss(a.double(), b.double(), reduction="sum")), rel=1e-12)
    assert R.relerr(ref["ga"], ga) < 1e-12
    same = L.mse(a, a, gs, vs, torch.float32)
    assert float(same["sum"]) == 0 and float(same["value"]) == 0 and R.same_bits(same["ga"], torch.zeros(n))


def test_luma_reference_is_metrics_luma():
    """Float32 coefficients against metrics.luma's Python floats: each is within 2^-25 of its decimal value and all are
    positive, so Y of an image in [0, 1] moves by at most 2^-25 of itself; the dB value against the oracle's psnr_y."""
    import metrics
    x_hat, x = L.psnr_images()
    assert x.shape == L.PSNR_IMAGE and x.shape[1] != x.shape[2] and x.shape[1] * x.shape[2] > L.CAP
    assert 0 <= float(x_hat.min()) and float(x_hat.max()) <= 1
    got, want = L.luma_of(x, F64), metrics.luma(x.double())
    assert got.shape == want.shape and bool(((got - want).abs() <= 2.0 ** -25 * want).all())
    db = float(L.psnr_db(x_hat, x, F64))
    assert 20 < db < 30 and db == pytest.approx(float(tp.psnr_y(x_hat.double(), x.double())), abs=1e-6)
    a, b = L.luma_inputs(257)
    want = (metrics.luma(a.double().view(3, 1, -1)) - metrics.luma(b.double().view(3, 1, -1))).pow(2).sum()
    assert float(L.luma_sqerr(a, b, F64)) == pytest.approx(float(want), rel=1e-6)


@pytest.mark.parametrize("M,N", [(1, 4), (37, 12), (333, 100), (64, 257)])
def test_colsum_reference_is_the_weighted_sum(M, N):
    X, w, out0 = L.colsum_inputs(M, N)
    assert int((w == 0).sum()) >= min(M - 1, 1) and (M == 1 or bool((w < 0).any()) and bool((w > 0).any()))
    assert R.relerr(L.colsum(X, w, out0, F64), out0.double() + (w.double()[:, None] * X.double()).sum(0)) < 1e-14
    assert R.relerr(L.colsum(X, None, out0, F64), out0.double() + X.double().sum(0)) < 1e-14


def test_colsum_row_block_model():
    """colsum_row_blocks restates launch_colsum's tiling: one row block up to 8 sweeps of the vector kernel's rows."""
    assert L.colsum_row_blocks(2048, 4, True) == 1 and L.colsum_row_blocks(2049, 4, True) == 2          # tpr 1: 256 x 8 rows
    assert L.colsum_row_blocks(37, 12, True) == 1 and L.colsum_row_blocks(2049, 12, True) == 5          # tpr 4: 64 x 8 rows
    assert L.colsum_row_blocks(8, 1024, True) == 1 and L.colsum_row_blocks(17, 1024, True) == 3         # tpr 256: 1 x 8 rows
    assert L.colsum_row_blocks(300, 1028, True) == 38
    assert L.colsum_row_blocks(73728, 32, True) == 72 and L.colsum_row_blocks(288, 8192, True) == 9
    assert L.colsum_row_blocks(5000, 300, True) == 79                                                  # rpb 16 -> 64
    assert L.colsum_row_blocks(16, 3, False) == 1 and L.colsum_row_blocks(50, 3, False) == 4
    assert L.colsum_row_blocks(40000, 7, False) == 1250 and L.colsum_row_blocks(1000, 128, False) == 63


# ---------------------------------------------------------------------------------------------- ref32 on the drawn cases
WORST = {}


def measured(family, dev, scale, floor):
    ref32 = float(dev) / max(float(scale), 1e-300)
    WORST[family] = max(WORST.get(family, 0.0), ref32)
    assert family in L.MEASURED_REF32, family
    assert 3 * ref32 < floor, (family, ref32)
    return ref32


def dev(r32, r64):
    return (r32.double() - r64.double()).abs().max()


def within(r32, r64, rel):
    """Every element of r32 within `rel` of its float64 value (no element here is small enough to be subnormal)."""
    return bool(((r32.double() - r64).abs() <= rel * r64.abs()).all())


def test_ref32_of_the_sure_families():
    cases = L.SURE_CASES + [L.SURE_NEGATIVE_TAU, L.SURE_JOINT, L.SURE_OFFSET]
    for case in cases:
        tau = -L.TAU if case is L.SURE_NEGATIVE_TAU else L.TAU
        _, _, r64, r32 = L.sure_case(*case, tau)
        got = (measured("sure div", dev(r32["div"], r64["div"]), r64["abs_div"], R.FLOOR),
               measured("sure mse", dev(r32["mse"], r64["mse"]), r64["mse"], R.FLOOR),
               measured("sure loss", dev(r32["loss"], r64["loss"]), r64["loss_scale"], R.FLOOR),
               measured("sure g1", dev(r32["g1"], r64["g1"]), r64["g1"].abs().max(), R.FLOOR))
        # g2 is three float32 roundings (1 / tau and two multiplies): within 2^-22 of float64 per element
        assert within(r32["g2"], r64["g2"], 2.0 ** -22)
        print(f"sure {case}: ref32 div {got[0]:.2e} mse {got[1]:.2e} loss {got[2]:.2e} g1 {got[3]:.2e}; "
              f"|div| / sum |terms| {abs(float(r64['div'])) / float(r64['abs_div']):.1e}")
    for family in ("sure div", "sure mse", "sure loss", "sure g1"):
        print(f"{family}: largest ref32 {WORST[family]:.2e} (floor {R.FLOOR:.0e})")


def test_ref32_of_the_mse_and_luma_families():
    for n in L.MSE_N:
        a, b = L.mse_inputs(n)
        for kind in L.MSE_SCALES:
            r64, r32 = (L.mse(a, b, *L.mse_scales(kind, n), dt) for dt in (F64, torch.float32))
            got = (measured("mse sum", dev(r32["sum"], r64["sum"]), r64["sum"], R.FLOOR),
                   measured("mse value", dev(r32["value"], r64["value"]), r64["value"], R.FLOOR))
            assert within(r32["ga"], r64["ga"], 2.0 ** -22)             # two roundings per element
            print(f"mse n={n} {kind}: ref32 sum {got[0]:.2e} value {got[1]:.2e}")
    for npix in L.LUMA_NPIX:
        a, b = L.luma_inputs(npix)
        r64 = L.luma_sqerr(a, b, F64)
        print(f"luma npix={npix}: ref32 {measured('luma sqerr', dev(L.luma_sqerr(a, b, torch.float32), r64), r64, R.FLOOR):.2e}")
    x_hat, x = L.psnr_images()
    r64 = L.luma_sqerr(x_hat.reshape(3, -1), x.reshape(3, -1), F64)
    r32 = L.luma_sqerr(x_hat.reshape(3, -1), x.reshape(3, -1), torch.float32)
    print(f"luma {L.PSNR_IMAGE}: ref32 {measured('luma sqerr', dev(r32, r64), r64, R.FLOOR):.2e}")
    for family in ("mse sum", "mse value", "luma sqerr"):
        print(f"{family}: largest ref32 {WORST[family]:.2e} (floor {R.FLOOR:.0e})")


def test_ref32_of_the_column_sums():
    for M, N in L.COLSUM_VEC + L.COLSUM_SCALAR + L.COLSUM_UNALIGNED:
        X, w, out0 = L.colsum_inputs(M, N)
        for family, ww in (("column sums", None), ("weighted column sums", w)):
            r64 = L.colsum(X, ww, out0, F64)
            ref32 = measured(family, dev(L.colsum(X, ww, out0, torch.float32), r64), r64.abs().max(), R.REDUCTION_FLOOR)
            print(f"{family} {M}x{N}: ref32 {ref32:.2e}")
    for family in ("column sums", "weighted column sums"):
        print(f"{family}: largest ref32 {WORST[family]:.2e} (floor {R.REDUCTION_FLOOR:.0e})")
