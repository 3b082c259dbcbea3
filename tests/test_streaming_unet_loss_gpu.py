"""The U-Net's bf16 / bf16x3 support kernels and the loss step's glue, one by one against tests/streaming_ref.py:
the residual fused into the LayerNorm backward (sei_ln_bwd_res, csrc/ln_kernels.hip), sei_cast_transpose_bf16 and
sei_weight_shadow_bf16 (csrc/bf16_support.hip), sei_split_bf16x2 / x3, sei_gelu_f32 and sei_mul_dgelu_f32
(csrc/bf16x3.hip), sei_concat2_f32, sei_scale_dev_f32, sei_add_scalars and sei_stack_axpy (csrc/draws.hip), sei_axpy and
sei_zero_ranges (csrc/loss_kernels.hip).

Bars (streaming_ref.py states them): exact = bit for bit against the same float32 operation on the CPU; float32 =
max(5e-6, 3 * ref32) of the float64 reference (2e-5 for column sums and LayerNorm parameter gradients). Every output lies
between two sentinel margins of its own allocation and is prefilled with the sentinel; input tails hold NaN.

Of test_layernorm_fwd_bwd's four odd shapes only (64, 3) and (10, 12) have sei_ln_bwd_part_count == 0 (float atomics,
the host adds the residual): (5, 700) and (50, 520) are multiples of 4 above 512 and take the two-pass kernels, which
fuse the residual. They stay in the list (the two-pass residual path has no other test), and (5, 701) and (30, 36) join
them for the wide and the grouped atomics kernels.

Measured on one MI355X (largest over the cases of a family; ref32 is the float32 CPU chain, bar the resulting bound):
    family                            ref32     bar       HIP deviation
    ln_bwd_res gx                     1.5e-7    5.0e-6    1.2e-7
    ln_bwd_res ggamma                 2.4e-7    2.0e-5    2.9e-7
    ln_bwd_res gbeta                  1.5e-7    2.0e-5    2.9e-7
    cast_transpose colsum             1.6e-7    2.0e-5    1.4e-7
    gelu                              3.0e-8    5.0e-6    1.1e-8
    mul_dgelu                         1.7e-7    5.0e-6    1.0e-7
    gelu at the fixed points (abs)    5.9e-9    5.0e-6    5.9e-9
    gelu' at the fixed points (abs)   6.5e-8    5.0e-6    3.6e-8
    axpy                              5.1e-8    5.0e-6    4.4e-8
    stack_axpy                        6.0e-8    5.0e-6    4.2e-8
So the floors, not measured bars, are what every family here is held to.
Everything else in this module is held bit for bit.
"""
import ctypes

import pytest
import torch

import streaming_ref as R

pytestmark = pytest.mark.gpu
X3_CAP = 4 * 4096 * 256                     # floats of one sweep of the bf16x3 streaming kernels (4096 workgroups, float4)
DRAWS_CAP = 4 * 2048 * 256                  # ... of concat2 / scale_dev / axpy / stack_axpy (2048 workgroups)


def native():
    import _native
    return _native


def refused(name, *args):
    N = native()
    with pytest.raises(N.NativeLibraryError):
        N.call(name, *args)
    torch.cuda.synchronize()


def randn(*shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def dev_scalar(v):
    return torch.tensor([v], dtype=torch.float32, device="cuda")


# ------------------------------------------------------------------------------------------------ sei_ln_bwd_res
LN_RES = [((500, 32), True), ((77, 128), True), ((300, 512), True), ((40, 2048), True), ((9, 8192), True),
          ((4099, 8), True), ((64, 3), False), ((10, 12), False), ((5, 700), True), ((50, 520), True),
          ((5, 701), False), ((30, 36), False)]


@pytest.mark.parametrize("shape,fused", LN_RES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_layer_norm_bwd_with_residual(shape, fused):
    """ops.layer_norm_bwd(..., res=r): gx = LN'(gy) + res and both parameter gradients (on top of random start values)
    against float64 autograd, one shape per kernel family; where sei_ln_bwd_part_count is 0 the host adds res and the
    entry point itself refuses one."""
    N = native()
    from models import _ops as ops
    rows, C = shape
    assert (N.lib().sei_ln_bwd_part_count(rows, C) > 0) == fused
    x, gamma, beta, gy, res = R.ln_inputs(rows, C, rows + C)
    _, mean, rstd = R.ln_fwd(x, gamma, beta, 1e-6, torch.float32)
    gx64, gg64, gb64 = R.ln_bwd_autograd(x, gamma, gy, 1e-6, res)
    gx32, gg32, gb32 = R.ln_bwd(x, gamma, mean, rstd, gy, torch.float32, res)
    gg0, gb0 = randn(C, seed=C), randn(C, seed=C + 1)
    gg, gb = R.Guarded(C), R.Guarded(C)
    gg.view.copy_(gg0); gb.view.copy_(gb0)
    resd = res.cuda()
    gx = ops.layer_norm_bwd(x.cuda(), gamma.cuda(), mean.cuda(), rstd.cuda(), gy.cuda(), gg.view, gb.view, res=resd)
    torch.cuda.synchronize()
    assert gg.intact() and gb.intact() and torch.equal(resd.cpu(), res)
    label = f"ln_bwd_res {rows}x{C}"
    R.hold32(label + " gx", gx, gx64, gx32)
    R.hold32(label + " ggamma", gg.view, gg0.double() + gg64, gg0 + gg32, R.REDUCTION_FLOOR)
    R.hold32(label + " gbeta", gb.view, gb0.double() + gb64, gb0 + gb32, R.REDUCTION_FLOOR)
    if not fused:
        out = torch.empty_like(resd)
        args = [t.cuda() for t in (x, gamma, mean, rstd, gy)]
        refused("sei_ln_bwd_res", *(t.data_ptr() for t in args), resd.data_ptr(), out.data_ptr(), gg.ptr(), gb.ptr(), rows, C,
                None, 0)


# ------------------------------------------------------------------------------------------------ sei_cast_transpose_bf16
CT_SHAPES = [(70, 130, 70), (70, 130, 128), (60, 50, 192), (64, 64, 64), (1, 5, 8)]


@pytest.mark.parametrize("outputs", ["x16+xt16+colsum", "x16", "xt16", "colsum", "x16+colsum"])
@pytest.mark.parametrize("Rr,C,ldt", CT_SHAPES)
def test_cast_transpose_bf16_from_float32(Rr, C, ldt, outputs):
    """x16 = bf16(x), xt16[:, :R] = bf16(x)^T with exact zeros in columns R .. ldt - 1 ((60, 50, 192): two whole 64-row
    tiles of padding, which must not add to the column sums again), colsum += column sums of the un-rounded x."""
    N = native()
    x = randn(Rr, C, seed=Rr + C + ldt)
    cs0 = randn(C, seed=ldt)
    x16, xt16, cs = R.Guarded((Rr, C), torch.bfloat16), R.Guarded((C, ldt), torch.bfloat16), R.Guarded(C)
    cs.view.copy_(cs0)
    want = outputs.split("+")
    xd = R.nan_tailed(x)
    N.call("sei_cast_transpose_bf16", xd.data_ptr(), 0, x16.ptr() if "x16" in want else None,
           xt16.ptr() if "xt16" in want else None, Rr, C, ldt, cs.ptr() if "colsum" in want else None)
    torch.cuda.synchronize()
    assert x16.intact() and xt16.intact() and cs.intact()
    untouched16 = lambda g: bool((g.view == R.SENTINEL).all())
    assert R.same_bits(x16.view, x.bfloat16()) if "x16" in want else untouched16(x16)
    if "xt16" in want:
        got = xt16.view.cpu()
        assert R.same_bits(got[:, :Rr], x.bfloat16().T.contiguous())
        assert R.same_bits(got[:, Rr:], torch.zeros((C, ldt - Rr), dtype=torch.bfloat16))
    else:
        assert untouched16(xt16)
    if "colsum" in want:
        R.hold32(f"cast_transpose colsum {Rr}x{C} ldt={ldt} [{outputs}]", cs.view, cs0.double() + x.double().sum(0),
                 cs0 + x.sum(0), R.REDUCTION_FLOOR)
    else:
        assert R.same_bits(cs.view, cs0)


@pytest.mark.parametrize("Rr,C,ldt", CT_SHAPES)
def test_cast_transpose_bf16_from_bf16(Rr, C, ldt):
    """bf16 input: the padded transpose only; a bf16 copy of a bf16 input is refused."""
    N = native()
    x = randn(Rr, C, seed=Rr + C + ldt + 1).bfloat16()
    xd = R.nan_tailed(x)
    xt16 = R.Guarded((C, ldt), torch.bfloat16)
    N.call("sei_cast_transpose_bf16", xd.data_ptr(), 1, None, xt16.ptr(), Rr, C, ldt, None)
    torch.cuda.synchronize()
    got = xt16.view.cpu()
    assert xt16.intact() and R.same_bits(got[:, :Rr], x.T.contiguous())
    assert R.same_bits(got[:, Rr:], torch.zeros((C, ldt - Rr), dtype=torch.bfloat16))
    x16 = R.Guarded((Rr, C), torch.bfloat16)
    refused("sei_cast_transpose_bf16", xd.data_ptr(), 1, x16.ptr(), xt16.ptr(), Rr, C, ldt, None)
    refused("sei_cast_transpose_bf16", xd.data_ptr(), 1, None, xt16.ptr(), Rr, C, Rr - 1, None)          # ldt < R


@pytest.mark.parametrize("outputs", ["w16+wt16", "w16", "wt16"])
@pytest.mark.parametrize("Rr,C", [(130, 70), (32, 128), (1, 3)])
def test_weight_shadow_bf16(Rr, C, outputs):
    N = native()
    w = randn(Rr, C, seed=Rr + C)
    w16, wt16 = R.Guarded((Rr, C), torch.bfloat16), R.Guarded((C, Rr), torch.bfloat16)
    wd = R.nan_tailed(w)
    N.call("sei_weight_shadow_bf16", wd.data_ptr(), w16.ptr() if "w16" in outputs.split("+") else None,
           wt16.ptr() if "wt16" in outputs else None, Rr, C)
    torch.cuda.synchronize()
    assert w16.intact() and wt16.intact()
    if "w16" in outputs.split("+"):
        assert R.same_bits(w16.view, w.bfloat16())
    else:
        assert bool((w16.view == R.SENTINEL).all())
    if "wt16" in outputs:
        assert R.same_bits(wt16.view, w.bfloat16().T.contiguous())
    else:
        assert bool((wt16.view == R.SENTINEL).all())


def test_weight_shadow_bf16_refuses_no_output():
    w = torch.zeros((4, 4), device="cuda")
    refused("sei_weight_shadow_bf16", w.data_ptr(), None, None, 4, 4)


# ------------------------------------------------------------------------------------------------ sei_split_bf16x2 / x3
@pytest.mark.parametrize("n", [4, 1028, X3_CAP + 8])
def test_split_bf16_planes(n):
    """x2: [hi | lo]; x3 pattern 0: [hi | hi | lo] (the A side), pattern 1: [hi | lo | hi] (the B side); hi = bf16(x),
    lo = bf16(x - float(hi)), over 2^-20 .. 2^20 with exact bf16 values and bf16 ties in front."""
    N = native()
    x = R.split_inputs(n, n)
    hi, lo = R.split_planes(x)
    xd = R.nan_tailed(x)
    p2 = R.Guarded((2, n), torch.bfloat16)
    N.call("sei_split_bf16x2", xd.data_ptr(), p2.ptr(), n)
    torch.cuda.synchronize()
    assert p2.intact() and R.same_bits(p2.view, torch.stack([hi, lo]))
    del p2
    for pattern, order in ((0, [hi, hi, lo]), (1, [hi, lo, hi])):
        p3 = R.Guarded((3, n), torch.bfloat16)
        N.call("sei_split_bf16x3", xd.data_ptr(), p3.ptr(), n, pattern)
        torch.cuda.synchronize()
        assert p3.intact() and R.same_bits(p3.view, torch.stack(order)), pattern
        del p3


def test_split_bf16_refusals():
    x, p = torch.zeros(16, device="cuda"), torch.zeros(48, device="cuda", dtype=torch.bfloat16)
    refused("sei_split_bf16x2", x.data_ptr(), p.data_ptr(), 6)
    refused("sei_split_bf16x3", x.data_ptr(), p.data_ptr(), 6, 0)
    refused("sei_split_bf16x3", x.data_ptr(), p.data_ptr(), 8, 2)


# ------------------------------------------------------------------------------------------------ sei_gelu_f32, sei_mul_dgelu_f32
@pytest.mark.parametrize("n", [1, 3, 4, 4099, X3_CAP + 4099])
def test_gelu_and_its_derivative(n):
    """Both kernels (the derivative in place, as used) in max-norm against F.gelu and its autograd in float64, and in
    absolute terms at the fixed points 0, -0.0, +-1e-30, +-0.5, +-6, +-13, +-40; n % 4 != 0 reaches the scalar tail."""
    N = native()
    x = R.gelu_inputs(n, n)
    d0 = randn(n, seed=n + 1)
    k = min(n, len(R.GELU_FIXED))
    d0[:k] = 1.0
    xd = R.nan_tailed(x)
    y, d = R.Guarded(n), R.Guarded(n)
    d.view.copy_(d0)
    N.call("sei_gelu_f32", xd.data_ptr(), y.ptr(), n)
    N.call("sei_mul_dgelu_f32", d.ptr(), xd.data_ptr(), n)
    torch.cuda.synchronize()
    assert y.intact() and d.intact() and R.same_bits(xd, x)
    y64, y32 = R.gelu(x, torch.float64), R.gelu(x, torch.float32)
    g64, g32 = R.mul_dgelu(d0, x, torch.float64), R.mul_dgelu(d0, x, torch.float32)
    R.hold32(f"gelu n={n}", y.view, y64, y32)
    R.hold32(f"mul_dgelu n={n}", d.view, g64, g32)
    R.hold32_abs(f"gelu fixed points n={n}", y.view[:k], y64[:k], y32[:k])
    R.hold32_abs(f"gelu' fixed points n={n}", d.view[:k], g64[:k], g32[:k])


# ------------------------------------------------------------------------------------------------ sei_concat2_f32
@pytest.mark.parametrize("na,nb", [(4, 0), (4, 4), (1000, 2000), (1_048_576 + 8, 1_200_000)])
def test_concat2(na, nb):
    """out = [a | b]; nb = 0 is a plain copy (b = NULL); 2,248,584 floats > 2048 x 256 float4: the loop's second turn."""
    N = native()
    a, b = randn(na, seed=na), randn(nb, seed=nb + 1)
    if na > 1_000_000:
        assert na + nb > DRAWS_CAP
    out = R.Guarded(na + nb)
    ad, bd = R.nan_tailed(a), R.nan_tailed(b) if nb else None
    N.call("sei_concat2_f32", ad.data_ptr(), na, N.ptr(bd), nb, out.ptr())
    torch.cuda.synchronize()
    assert out.intact() and R.same_bits(out.view, torch.cat([a, b]))


# ------------------------------------------------------------------------------------------------ sei_scale_dev_f32, sei_add_scalars
@pytest.mark.parametrize("scalar", [0.0, -1.75, 0.37])
@pytest.mark.parametrize("n", [4, 1000, DRAWS_CAP + 4096])
def test_scale_dev(n, scalar):
    """out = x * (*scalar) with the scalar read from device memory: one float32 multiply."""
    N = native()
    x, s = randn(n, seed=n), dev_scalar(scalar)
    out = R.Guarded(n)
    xd = R.nan_tailed(x)
    N.call("sei_scale_dev_f32", xd.data_ptr(), s.data_ptr(), out.ptr(), n)
    torch.cuda.synchronize()
    assert out.intact() and R.same_bits(out.view, x * s.cpu())


@pytest.mark.parametrize("a,b", [(0.0, 0.0), (0.1, 0.2), (-1.5, 1.5), (3.25, -7.125), (-0.0, -0.0), (1e-30, -3e30)])
def test_add_scalars(a, b):
    N = native()
    ad, bd, out = dev_scalar(a), dev_scalar(b), R.Guarded(1)
    N.call("sei_add_scalars", ad.data_ptr(), bd.data_ptr(), out.ptr())
    torch.cuda.synchronize()
    assert out.intact() and R.same_bits(out.view, ad.cpu() + bd.cpu())


# ------------------------------------------------------------------------------------------------ sei_axpy, sei_stack_axpy
def axpy_refs(a, b, alpha):
    al = torch.tensor(alpha, dtype=torch.float32)
    return a.double() + al.double() * b.double(), a + al * b


@pytest.mark.parametrize("n", [5, 1002, 4099, 4, DRAWS_CAP + 4099])
def test_axpy(n):
    """out = a + alpha b (one FMA per element): n % 4 = 1, 2, 3 reach the scalar tail; the last n is past the grid cap."""
    N = native()
    a, b, alpha = randn(n, seed=n), randn(n, seed=n + 1), -0.37
    out = R.Guarded(n)
    ad, bd = R.nan_tailed(a), R.nan_tailed(b)
    N.call("sei_axpy", ad.data_ptr(), bd.data_ptr(), alpha, out.ptr(), n)
    torch.cuda.synchronize()
    assert out.intact()
    R.hold32(f"axpy n={n}", out.view, *axpy_refs(a, b, alpha))


@pytest.mark.parametrize("n", [4, 1000, 6 * 48 * 48 * 3, DRAWS_CAP + 4096])
def test_stack_axpy(n):
    """out[:n] is a, bit for bit; out[n:] is what sei_axpy writes for the same operands, bit for bit; both against float64."""
    N = native()
    a, b, alpha = randn(n, seed=n), randn(n, seed=n + 1), 0.73
    ad, bd = R.nan_tailed(a), R.nan_tailed(b)
    out, single = R.Guarded((2, n)), R.Guarded(n)
    N.call("sei_stack_axpy", ad.data_ptr(), bd.data_ptr(), alpha, out.ptr(), n)
    N.call("sei_axpy", ad.data_ptr(), bd.data_ptr(), alpha, single.ptr(), n)
    torch.cuda.synchronize()
    assert out.intact() and single.intact()
    assert R.same_bits(out.view[0], a) and R.same_bits(out.view[1], single.view)
    r64, r32 = axpy_refs(a, b, alpha)
    R.hold32(f"stack_axpy n={n}", out.view, torch.stack([a.double(), r64]), torch.stack([a, r32]))
    refused("sei_stack_axpy", ad.data_ptr(), bd.data_ptr(), alpha, out.ptr(), n + 2)                 # n % 4 != 0


# ------------------------------------------------------------------------------------------------ sei_zero_ranges
ZERO_N = 1_300_000
ZERO_RANGES = [
    [(5, 3)],
    [(0, 0), (7, 1_100_000), (ZERO_N - 9, 9)],                                   # one range past 4096 x 256 elements
    [(0, 0), (3, 5), (8, 4), (12, 0), (101, 7), (1000, 256), (1256, 1), (ZERO_N, 0)],        # adjacent, odd, empty
    [(0, 4), (4, 0), (ZERO_N - 1, 1)],
]


def pairs_array(pairs):
    flat = [v for p in pairs for v in p]
    return (ctypes.c_ulonglong * len(flat))(*flat)


@pytest.mark.parametrize("pairs", ZERO_RANGES, ids=lambda p: f"{len(p)}ranges")
def test_zero_ranges(pairs):
    """Exactly the named elements become 0 and every other element keeps its bits."""
    N = native()
    base0 = randn(ZERO_N, seed=len(pairs))
    base0[base0 == 0] = 1.0
    base = R.Guarded(ZERO_N)
    base.view.copy_(base0)
    N.call("sei_zero_ranges", base.ptr(), pairs_array(pairs), len(pairs))
    torch.cuda.synchronize()
    mask = R.zero_ranges_mask(ZERO_N, pairs)
    assert int(mask.sum()) == sum(length for _, length in pairs)
    assert base.intact() and R.same_bits(base.view, torch.where(mask, torch.zeros(()), base0))


def test_zero_ranges_empty_and_refused():
    """All lengths 0: success, nothing written; 0 or 9 ranges are refused."""
    N = native()
    base0 = randn(64, seed=1)
    base = R.Guarded(64)
    base.view.copy_(base0)
    N.call("sei_zero_ranges", base.ptr(), pairs_array([(0, 0), (17, 0), (64, 0)]), 3)
    torch.cuda.synchronize()
    assert base.intact() and R.same_bits(base.view, base0)
    nine = pairs_array([(k, 1) for k in range(9)])
    refused("sei_zero_ranges", base.ptr(), nine, 9)
    refused("sei_zero_ranges", base.ptr(), nine, 0)
    assert R.same_bits(base.view, base0)
