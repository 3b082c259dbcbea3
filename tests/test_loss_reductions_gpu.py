"""The loss reductions and the column sums, entry point by entry point through the C ABI against
tests/loss_reduction_ref.py: sei_sure_loss, sei_sure_terms, sei_mse_loss, sei_mse_terms and sei_luma_sqerr
(csrc/loss_kernels.hip: two-stage reductions of min(256, ceil(n / 1024)) workgroups, so n = 262144 is where the grid-stride
loop starts to do the work -- the regime metrics.psnr_fn runs in on every full-size image), sei_colsum_f32 and
sei_colsum_weighted_f32 (csrc/reduce_kernels.hip: a float4 kernel, a scalar kernel and a dispatch on N % 4 and the
pointer), and models/_ops.py's colsum_into on the host.

Bars (loss_reduction_ref.py and streaming_ref.py state them): ga = scale * (a - b) and g2 = (c_div * b) * inv_tau bit for
bit against the same float32 operations on the CPU; g1 (an fmaf in the kernel) to max(5e-6, 3 * ref32) of float64; every
scalar sum and loss value to the same bar relative to the float64 sum of the ABSOLUTE terms; column sums to
max(2e-5, 3 * ref32) of the largest float64 column. Every output and every workspace (sized exactly) lies between two
sentinel margins of its own allocation and is prefilled with the sentinel, input tails hold NaN, and the loss kernels,
which use no atomics, must return the same bits when called again.

Measured on one MI355X (largest over the cases of a family; ref32 is the float32 CPU chain, bar the resulting bound):
    family                            ref32     bar       HIP deviation
    sure div sum   (of sum |terms|)   8.0e-8    5.0e-6    8.0e-8
    sure mse sum                      1.2e-7    5.0e-6    5.0e-8
    sure loss value (of its scale)    8.0e-8    5.0e-6    4.6e-8
    sure g1                           1.1e-7    5.0e-6    1.1e-7
    mse sum                           8.6e-8    5.0e-6    4.8e-8
    mse value                         1.2e-7    5.0e-6    9.6e-8
    luma sqerr                        7.2e-7    5.0e-6    7.2e-7
    psnr_fn, 3 x 531 x 497 (dB)       --        3.6e-5    2.7e-6
    column sums                       5.7e-7    2.0e-5    6.4e-7
    weighted column sums              1.8e-7    2.0e-5    5.5e-7
So the floors, not measured bars, are what every family here is held to. (The one- and few-element cases set most of these
figures: there a single rounding is the whole deviation, and the kernel makes the same one as the CPU chain.) g2 and ga are
held bit for bit, as is everything this module compares between two calls.

By hand, on a scratch copy of the kernels (not kept): H and W swapped in sure_terms_kernel's masks fails exactly the
non-square SURE cases; 255 workgroups under the 256-workgroup stride fails exactly the cases of 262144 elements and more
(SURE, mse, luma, psnr_fn); `4 * q <= N` in colsum_vec_kernel fails exactly the 12-, 100-, 300- and 1028-column float4 cases.
"""
import pytest
import torch

import loss_reduction_ref as L
import streaming_ref as R

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
BLOCKS = 256                                # SEI_REDUCE_BLOCKS (include/sei_hip.h): partial sums per reduced quantity


def native():
    import _native
    assert _native.SEI_REDUCE_BLOCKS == BLOCKS
    return _native


def refused(name, *args):
    N = native()
    with pytest.raises(N.NativeLibraryError):
        N.call(name, *args)
    torch.cuda.synchronize()


def untouched(*guards):
    """Nothing was written: margins and the outputs proper still hold the sentinel."""
    return all(g.intact() and bool((g.view == R.SENTINEL).all()) for g in guards)


def ids(case):
    return "x".join(str(int(v)) if isinstance(v, bool) else str(v) for v in case) if isinstance(case, tuple) else None


class Out:
    """A Guarded output of n floats whose first element lies `lead` floats behind the front margin: lead = 1 puts it 4
    bytes off the 16-byte grid, and the skipped elements must keep the sentinel as the margins do."""

    def __init__(self, shape, lead=0):
        n = int(torch.Size(shape if isinstance(shape, (tuple, list)) else (shape,)).numel())
        self.guard, self.lead = R.Guarded(n + lead), lead
        self.view = self.guard.view[lead:].view(shape)

    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        return self.guard.intact() and bool((self.guard.view[:self.lead] == R.SENTINEL).all())


# ------------------------------------------------------------------------------------------------ sei_sure_loss, sei_sure_terms
def run_sure(entry, case, tau=L.TAU, joint=False, lead=0):
    """One call on fresh buffers -> (out (3 or 2 floats), g1, g2) on the CPU after the margins were checked."""
    N = native()
    planes, H, W, md, mm, border_b = case
    y, y1, y2, b = L.sure_inputs(*case)
    c_mse, c_div, cst = L.sure_constants(planes, H, W, md, mm)
    put = (lambda t: R.nan_framed(t, lead)) if lead else R.nan_tailed
    yd, bd = put(y), put(b)
    if joint:                                   # y1 | y2 and g1 | g2 as the halves of one tensor of 2 * planes images
        y12 = put(torch.stack([y1, y2]))
        g12 = Out((2, planes, H, W), lead)
        p1, p2, q1, q2, outs = y12[0].data_ptr(), y12[1].data_ptr(), g12.view[0].data_ptr(), g12.view[1].data_ptr(), [g12]
        assert p2 - p1 == 4 * y.numel() and q2 - q1 == 4 * y.numel()
    else:
        y1d, y2d, g1, g2 = put(y1), put(y2), Out((planes, H, W), lead), Out((planes, H, W), lead)
        p1, p2, q1, q2, outs = y1d.data_ptr(), y2d.data_ptr(), g1.ptr(), g2.ptr(), [g1, g2]
    assert not lead or all(p % 16 == 4 * lead for p in (yd.data_ptr(), bd.data_ptr(), p1, q1))
    loss = entry == "sei_sure_loss"
    out, work = Out(3 if loss else 2, lead), Out(2 * BLOCKS, lead)
    head = (yd.data_ptr(), p1, p2, bd.data_ptr(), planes, H, W, md, mm, tau, c_mse, c_div)
    N.call(entry, *head, *((cst,) if loss else ()), out.ptr(), q1, q2, work.ptr())
    torch.cuda.synchronize()
    assert out.intact() and work.intact() and all(g.intact() for g in outs), (entry, case)
    assert R.same_bits(yd, y) and R.same_bits(bd, b)
    if joint:
        return out.view.cpu(), g12.view[0].cpu(), g12.view[1].cpu()
    return out.view.cpu(), g1.view.cpu(), g2.view.cpu()


def hold_sure(label, got, r64, r32):
    out, g1, g2 = got
    devs = {"sure div": R.hold32_on(label + " div sum", out[0], r64["div"], r32["div"], r64["abs_div"]),
            "sure mse": R.hold32_on(label + " mse sum", out[1], r64["mse"], r32["mse"], r64["mse"])}
    if out.numel() == 3:
        devs["sure loss"] = R.hold32_on(label + " loss", out[2], r64["loss"], r32["loss"], r64["loss_scale"])
    assert R.same_bits(g2, r32["g2"]), label + ": g2 is (c_div * b) * (1.0f / tau) inside the interior and +0.0 outside"
    devs["sure g1"] = R.hold32(label + " g1", g1, r64["g1"], r32["g1"])
    return devs


@pytest.mark.parametrize("case", L.SURE_CASES, ids=ids)
def test_sure_loss_grid(case):
    """All three scalars and both gradients (written everywhere: the zeros outside the interiors come from the kernel) on
    non-square images, unequal margins, a one-pixel interior and element counts up to, at and past the grid cap; called
    again, the same bits."""
    _, _, r64, r32 = L.sure_case(*case)
    got = run_sure("sei_sure_loss", case)
    hold_sure(f"sure_loss {ids(case)}", got, r64, r32)
    again = run_sure("sei_sure_loss", case)
    assert all(R.same_bits(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("case", L.SURE_TERMS_SUBSET, ids=ids)
def test_sure_terms_is_the_first_stage_of_sure_loss(case):
    """sei_sure_terms shares stage 1: its two sums are out3[:2] and its gradients those of sei_sure_loss, bit for bit."""
    _, _, r64, r32 = L.sure_case(*case)
    terms, loss = run_sure("sei_sure_terms", case), run_sure("sei_sure_loss", case)
    hold_sure(f"sure_terms {ids(case)}", terms, r64, r32)
    assert R.same_bits(terms[0], loss[0][:2]) and R.same_bits(terms[1], loss[1]) and R.same_bits(terms[2], loss[2])


def test_sure_loss_negative_tau():
    case = L.SURE_NEGATIVE_TAU
    _, _, r64, r32 = L.sure_case(*case, -L.TAU)
    assert float(r64["div"]) == -float(L.sure_case(*case)[2]["div"])
    hold_sure(f"sure_loss {ids(case)} tau<0", run_sure("sei_sure_loss", case, tau=-L.TAU), r64, r32)


def test_sure_loss_joint_layout_and_storage_offset():
    """y1 | y2 and g1 | g2 as the two halves of one 2B-image tensor (what ProposedLoss passes), and every operand, output
    and the workspace 4 bytes off the 16-byte grid: the same bits as the plain aligned call."""
    for case, kw in ((L.SURE_JOINT, dict(joint=True)), (L.SURE_OFFSET, dict(lead=1)), (L.SURE_JOINT, dict(joint=True, lead=1))):
        _, _, r64, r32 = L.sure_case(*case)
        got, plain = run_sure("sei_sure_loss", case, **kw), run_sure("sei_sure_loss", case)
        hold_sure(f"sure_loss {ids(case)} {kw}", got, r64, r32)
        assert all(R.same_bits(a, b) for a, b in zip(got, plain)), kw


@pytest.mark.parametrize("entry", ["sei_sure_loss", "sei_sure_terms"])
def test_sure_refusals(entry):
    """An empty interior (2 * margin == H or W, for either margin), tau == 0 and planes == 0: NativeLibraryError, and
    nothing is written."""
    loss = entry == "sei_sure_loss"
    H, W = 8, 6
    t = R.nan_tailed(torch.rand((2, H, W)))
    out, g1, g2, work = R.Guarded(3 if loss else 2), R.Guarded((2, H, W)), R.Guarded((2, H, W)), R.Guarded(2 * BLOCKS)

    def call(planes, h, w, md, mm, tau):
        assert planes * h * w <= t.numel()
        return (t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), planes, h, w, md, mm, tau, 0.01, 0.02) + \
            ((0.005,) if loss else ()) + (out.ptr(), g1.ptr(), g2.ptr(), work.ptr())

    for bad in ((2, H, W, 3, 0, 0.01), (2, H, W, 0, 3, 0.01),           # 2 * margin == W
                (2, W, H, 3, 0, 0.01), (2, W, H, 0, 3, 0.01),           # 2 * margin == H
                (1, H, H, 4, 4, 0.01), (2, H, W, 0, 0, 0.0), (0, H, W, 0, 0, 0.01)):
        refused(entry, *call(*bad))
        assert untouched(out, g1, g2, work), bad
    native().call(entry, *call(2, H, W, 2, 2, 0.01))                    # the same buffers, one step inside the bound
    torch.cuda.synchronize()
    assert bool((g1.view != R.SENTINEL).all()) and bool((g2.view != R.SENTINEL).all()) and g1.intact() and g2.intact()


# ------------------------------------------------------------------------------------------------ sei_mse_loss, sei_mse_terms
def run_mse(entry, a, b, scales, lead=(0, 0, 0)):
    """-> (out (2 or 1 floats), ga) on the CPU; lead: the storage offsets of a, b and (ga, out, work) in floats."""
    N = native()
    n = a.numel()
    ad, bd = R.nan_framed(a, lead[0]), R.nan_framed(b, lead[1])
    loss = entry == "sei_mse_loss"
    out, ga, work = Out(2 if loss else 1, lead[2]), Out(n, lead[2]), Out(BLOCKS, lead[2])
    N.call(entry, ad.data_ptr(), bd.data_ptr(), n, *(scales if loss else scales[:1]), out.ptr(), ga.ptr(), work.ptr())
    torch.cuda.synchronize()
    assert out.intact() and ga.intact() and work.intact(), (entry, n)
    assert R.same_bits(ad, a) and R.same_bits(bd, b)
    return out.view.cpu(), ga.view.cpu()


@pytest.mark.parametrize("kind", L.MSE_SCALES)
@pytest.mark.parametrize("n", L.MSE_N)
def test_mse_loss_and_terms(n, kind):
    """sum (a - b)^2 and value_scale times it against float64; ga = grad_scale * (a - b), and the value as one multiply
    of the kernel's own sum, bit for bit; with a, b, ga, out and work at 4-byte storage offsets the same bits (the kernel
    asks for no alignment); sei_mse_terms returns the same sum and gradient."""
    a, b = L.mse_inputs(n)
    scales = L.mse_scales(kind, n)
    r64, r32 = L.mse(a, b, *scales, F64), L.mse(a, b, *scales, F32)
    out, ga = run_mse("sei_mse_loss", a, b, scales)
    label = f"mse_loss n={n} {kind}"
    R.hold32_on(label + " sum", out[0], r64["sum"], r32["sum"], r64["sum"])
    R.hold32_on(label + " value", out[1], r64["value"], r32["value"], r64["value"])
    assert R.same_bits(ga, r32["ga"]) and R.same_bits(out[1:], L.f32(scales[1]) * out[:1])
    for lead in ((1, 3, 2), (0, 1, 0)):
        off = run_mse("sei_mse_loss", a, b, scales, lead)
        assert R.same_bits(off[0], out) and R.same_bits(off[1], ga), lead
    terms = run_mse("sei_mse_terms", a, b, scales, (3, 0, 1))
    assert R.same_bits(terms[0], out[:1]) and R.same_bits(terms[1], ga)


@pytest.mark.parametrize("n", [1, 257, L.CAP + 1])
def test_mse_of_equal_operands_is_exactly_zero(n):
    a, _ = L.mse_inputs(n)
    for entry in ("sei_mse_loss", "sei_mse_terms"):
        out, ga = run_mse(entry, a, a.clone(), L.mse_scales("w=0.1", n), (1, 2, 3))
        assert R.same_bits(out, torch.zeros(out.numel())) and R.same_bits(ga, torch.zeros(n)), entry


def test_mse_and_luma_refuse_no_elements():
    t = R.nan_tailed(torch.rand(12))
    out, ga, work = R.Guarded(2), R.Guarded(4), R.Guarded(BLOCKS)
    refused("sei_mse_loss", t.data_ptr(), t.data_ptr(), 0, 0.5, 0.25, out.ptr(), ga.ptr(), work.ptr())
    refused("sei_mse_terms", t.data_ptr(), t.data_ptr(), 0, 0.5, out.ptr(), ga.ptr(), work.ptr())
    refused("sei_luma_sqerr", t.data_ptr(), t.data_ptr(), 0, out.ptr(), work.ptr())
    assert untouched(out, ga, work)


# ------------------------------------------------------------------------------------------------ sei_luma_sqerr
@pytest.mark.parametrize("npix", L.LUMA_NPIX)
def test_luma_sqerr(npix):
    """sum over the pixels of (Y(a) - Y(b))^2 for planar RGB images in [0, 1], up to, at and past the grid cap; the
    reference applies the kernel's float32 coefficients in float64. Called at a storage offset, the same bits."""
    N = native()
    a, b = L.luma_inputs(npix)
    r64, r32 = L.luma_sqerr(a, b, F64), L.luma_sqerr(a, b, F32)
    got = []
    for lead in (0, 1):
        ad, bd = R.nan_framed(a, lead), R.nan_framed(b, 2 * lead)
        out, work = Out(1, lead), Out(BLOCKS, lead)
        N.call("sei_luma_sqerr", ad.data_ptr(), bd.data_ptr(), npix, out.ptr(), work.ptr())
        torch.cuda.synchronize()
        assert out.intact() and work.intact() and R.same_bits(ad, a) and R.same_bits(bd, b)
        got.append(out.view.cpu())
    R.hold32_on(f"luma_sqerr npix={npix}", got[0][0], r64, r32, r64)
    assert R.same_bits(got[0], got[1])


def test_psnr_fn_on_a_full_size_image():
    """metrics.psnr_fn on a non-square 3 x 531 x 497 image (263907 pixels: the capped grid) against the float64 formula in
    dB. The bar: d(dB) = (10 / ln 10) d(sum) / sum, the sum held to max(5e-6, 3 * ref32) as above, and the float32
    division, reciprocal, log10 and multiply behind the kernel within 8 ulp of the dB value in all."""
    import math
    import metrics
    x_hat, x = L.psnr_images()
    flat = lambda t: t.reshape(3, -1)
    s64, s32 = L.luma_sqerr(flat(x_hat), flat(x), F64), L.luma_sqerr(flat(x_hat), flat(x), F32)
    ref32 = float((s32.double() - s64).abs() / s64)
    db64 = float(L.psnr_db(x_hat, x, F64))
    got = float(metrics.psnr_fn(R.nan_tailed(x_hat), R.nan_tailed(x)))
    bound = 10 / math.log(10) * R.bar(ref32) + 8 * 2.0 ** -24 * abs(db64)
    print(f"psnr_fn {L.PSNR_IMAGE}: {got:.6f} dB, float64 {db64:.6f} dB, apart {abs(got - db64):.2e} dB, ref32 of the sum "
          f"{ref32:.2e}, bar {bound:.2e} dB")
    assert abs(got - db64) <= bound


# ------------------------------------------------------------------------------------------------ sei_colsum_f32 / _weighted_f32
def run_colsum(M, N_, weighted, lead=0):
    """out0 + the (weighted) column sums on the CPU, the margins checked."""
    N = native()
    X, w, out0 = L.colsum_inputs(M, N_)
    Xd, wd = R.nan_framed(X, lead), R.nan_framed(w, lead)
    assert Xd.data_ptr() % 16 == 4 * lead
    out = Out(N_, lead)
    out.view.copy_(out0)
    if weighted:
        N.call("sei_colsum_weighted_f32", Xd.data_ptr(), wd.data_ptr(), out.ptr(), M, N_)
    else:
        N.call("sei_colsum_f32", Xd.data_ptr(), out.ptr(), M, N_)
    torch.cuda.synchronize()
    assert out.intact() and R.same_bits(Xd, X) and R.same_bits(wd, w), (M, N_, weighted, lead)
    return out.view.cpu()


COLSUM_CASES = [(M, N_, 0) for M, N_ in L.COLSUM_VEC + L.COLSUM_SCALAR] + [(M, N_, 1) for M, N_ in L.COLSUM_UNALIGNED]


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("M,N_,lead", COLSUM_CASES, ids=lambda v: str(v))
def test_colsum(M, N_, lead, weighted):
    """out[n] += sum_m (w[m]) X[m, n] on top of random values (a kernel that overwrote them would be told from one that
    adds), signed weights with zeros among them: the float4 kernel (dead quads, a second column block, the 8-sweep loop
    and its tail), the scalar kernel (idle threads, a second column block) and the dispatch's fall-back to it for
    N % 4 == 0 on an unaligned pointer. Where one row block covers M every column gets one atomic: the same bits again."""
    X, w, out0 = L.colsum_inputs(M, N_)
    ww = w if weighted else None
    got = run_colsum(M, N_, weighted, lead)
    R.hold32(f"colsum {'weighted ' if weighted else ''}{M}x{N_} lead={lead}", got, L.colsum(X, ww, out0, F64),
             L.colsum(X, ww, out0, F32), R.REDUCTION_FLOOR)
    if L.colsum_row_blocks(M, N_, aligned=not lead) == 1:
        assert R.same_bits(run_colsum(M, N_, weighted, lead), got)


def test_colsum_refusals():
    X, w = R.nan_tailed(torch.rand((4, 8))), R.nan_tailed(torch.rand(4))
    out = R.Guarded(8)
    refused("sei_colsum_f32", X.data_ptr(), out.ptr(), 0, 8)
    refused("sei_colsum_f32", X.data_ptr(), out.ptr(), 4, 0)
    refused("sei_colsum_weighted_f32", X.data_ptr(), w.data_ptr(), out.ptr(), 0, 8)
    refused("sei_colsum_weighted_f32", X.data_ptr(), w.data_ptr(), out.ptr(), 4, 0)
    refused("sei_colsum_weighted_f32", X.data_ptr(), None, out.ptr(), 4, 8)
    assert untouched(out)


# ------------------------------------------------------------------------------------------------ models/_ops.py: colsum_into
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_colsum_into_on_the_host(weighted):
    """colsum_into hands the kernel data_ptr() and the shape: a column slice X[:, :N] of a wider matrix (rows N + 4
    apart) must give the slice's sums or raise, never the sums of the first M * N floats; an accumulator of another
    length, or a row-weight vector of another length, must raise; nothing is written when it raises. Contiguous operands
    at a storage offset are served."""
    from models import _ops as ops
    M, N_ = 37, 12
    X, w, out0 = L.colsum_inputs(M, N_)
    wide = R.nan_tailed(torch.cat([X, 100 + torch.rand((M, 4))], dim=1))
    wd = R.nan_tailed(w) if weighted else None
    r64, r32 = (L.colsum(X, w if weighted else None, out0, dt) for dt in (F64, F32))
    acc = R.Guarded(N_)
    acc.view.copy_(out0)
    sliced = wide[:, :N_]
    assert not sliced.is_contiguous()
    try:
        ops.colsum_into(acc.view, sliced, row_weight=wd)
    except (ValueError, native().NativeLibraryError):
        torch.cuda.synchronize()
        assert acc.intact() and R.same_bits(acc.view, out0)
    else:
        torch.cuda.synchronize()
        assert acc.intact()
        R.hold32(f"colsum_into of a column slice {M}x{N_}", acc.view, r64, r32, R.REDUCTION_FLOOR)
    Xd = R.nan_framed(X, 1)
    for bad_acc in (R.Guarded(N_ + 4), R.Guarded(N_ - 1)):
        with pytest.raises(ValueError):
            ops.colsum_into(bad_acc.view, Xd, row_weight=wd)
        torch.cuda.synchronize()
        assert untouched(bad_acc)
    with pytest.raises(ValueError):
        ops.colsum_into(acc.view, Xd.view(-1), row_weight=wd)
    if weighted:
        with pytest.raises(ValueError):
            ops.colsum_into(acc.view, Xd, row_weight=wd[:-1])
    acc.view.copy_(out0)
    ops.colsum_into(acc.view, Xd, row_weight=wd)
    torch.cuda.synchronize()
    assert acc.intact()
    R.hold32(f"colsum_into at a storage offset {M}x{N_}", acc.view, r64, r32, R.REDUCTION_FLOOR)
