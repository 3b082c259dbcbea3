"""tests/streaming_ref.py on the CPU: the constructions that the streaming-kernel GPU tests compare with are anchored to
F.pad, to autograd in float64 and to the float32 / bfloat16 formats before any kernel is held to them, and `ref32` of
every float32 family is measured on the inputs those tests draw: below a third of the floor, so the floor is the bar
(the one family where it is not is named, with its value)."""
import pytest
import torch
import torch.nn.functional as F

import streaming_ref as R

LN_C = (180, 4, 60, 64, 252, 256)


@pytest.mark.parametrize("B,H,W,C,Cp,guard", [(1, 1, 1, 4, 8, 0), (2, 3, 5, 60, 64, 7), (1, 8, 8, 180, 192, 10),
                                              (3, 2, 9, 64, 64, 3)])
def test_padded_grid_is_f_pad(B, H, W, C, Cp, guard):
    x = torch.randn((B, H, W, C), generator=torch.Generator().manual_seed(C + guard))
    want = F.pad(x, (0, Cp - C, 1, 1, 1, 1)).view(-1, Cp)
    want = F.pad(want, (0, 0, guard, guard))
    got = R.padded_grid(x, guard, Cp)
    assert R.same_bits(got, want)
    assert R.same_bits(R.padded_grid(x.bfloat16(), guard, Cp), want.bfloat16())
    if Cp > C:
        ones = R.padded_grid(x, guard, Cp, ones_col=True)
        assert bool((ones[:, C] == 1).all()) and ones.shape == want.shape
        ones[:, C] = 0
        assert R.same_bits(ones, want)
    else:
        with pytest.raises(AssertionError):
            R.padded_grid(x, guard, Cp, ones_col=True)


@pytest.mark.parametrize("C", LN_C)
def test_layernorm_formulas_are_autograd(C):
    """ln_fwd is F.layer_norm and ln_bwd (from float64 statistics) is its torch.autograd.grad, to 1e-12 in float64."""
    x, gamma, beta, gy, res = R.ln_inputs(50, C, C, special_rows=True)
    y, mean, rstd = R.ln_fwd(x, gamma, beta, 1e-5, torch.float64)
    assert R.relerr(y, F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5)) < 1e-12
    assert R.same_bits(y[-1], beta.double()) and float(rstd[-1]) == pytest.approx(1e-5 ** -0.5, rel=1e-12)
    for r in (None, res):
        want = R.ln_bwd_autograd(x, gamma, gy, 1e-5, r)
        got = R.ln_bwd(x, gamma, mean, rstd, gy, torch.float64, r)
        for a, b in zip(got, want):
            assert R.relerr(a, b) < 1e-12


@pytest.mark.parametrize("C", LN_C)
def test_constant_row_is_exact_in_float32(C):
    """The constant row's float32 mean is the constant, by division and by the reciprocal: y = beta exactly."""
    c = R.exact_constant(C)
    row = torch.full((1, C), c)
    assert float(row.sum() / C) == c and float(row.sum() * (torch.tensor(1.0) / C)) == c
    y, mean, rstd = R.ln_fwd(row, torch.randn(C), torch.arange(C, dtype=torch.float32), 1e-5, torch.float32)
    assert float(mean) == c and torch.equal(y[0], torch.arange(C, dtype=torch.float32))


def test_split_planes_reconstruct_x():
    """hi + lo recovers x to 2^-16 relative (two bf16 mantissas), exact bf16 values leave a zero remainder, ties round to
    even, and the planted values are there."""
    x = R.split_inputs(4100, 3)
    hi, lo = R.split_planes(x)
    assert float(x.abs().max()) < 2.0 ** 21 and float(x[x != 0].abs().min()) >= 2.0 ** -21
    err = (hi.double() + lo.double() - x.double()).abs()
    assert bool((err <= 2.0 ** -16 * x.double().abs()).all())
    assert bool((lo[:8].float() == 0).all()) and R.same_bits(hi[:8].float(), x[:8])
    ties = x[8:14].view(torch.int32)
    assert bool(((ties & 0xFFFF) == 0x8000).all())
    even = (hi[8:14].view(torch.int16).to(torch.int32) & 1) == 0
    assert bool(even.all())
    assert R.split_inputs(4, 3).shape == (4,)


def test_scaled_cast_rounds_the_float32_product():
    x, s = torch.randn(7, 12), torch.rand(7)
    v, v16 = R.scaled_cast(x, s)
    assert R.same_bits(v, (x.double() * s.double()[:, None]).float()) and R.same_bits(v16, v.bfloat16())
    assert R.same_bits(R.scaled_cast(x)[1], x.bfloat16())


def test_maps_and_ranges():
    m = R.index_map(1000, 1050, 1)
    used = m[m >= 0]
    assert used.unique().numel() == used.numel() and 50 < int((m < 0).sum()) < 150 and int(m.max()) < 1050
    src, dst = torch.randn(1050), torch.randn(1050)
    packed = R.pack_ref(src, m)
    assert bool((packed[m < 0] == 0).all()) and torch.equal(packed[m >= 0], src[used.long()])
    out = R.unpack_add_ref(src[:1000], m, dst)
    touched = torch.zeros(1050, dtype=torch.bool)
    touched[used.long()] = True
    assert R.same_bits(out[~touched], dst[~touched]) and int((out != dst).sum()) > 800
    mask = R.zero_ranges_mask(20, [(0, 0), (3, 2), (5, 1), (20, 0)])
    assert mask.nonzero().flatten().tolist() == [3, 4, 5]


def test_leaky_branches():
    v = torch.tensor([-2.0, -0.0, 0.0, 3.0])
    assert R.same_bits(R.leaky(v), torch.tensor([-2.0 * torch.tensor(0.01).item(), -0.0, 0.0, 3.0]).float())
    assert R.leaky_gate(v).tolist() == pytest.approx([0.01, 0.01, 0.01, 1.0], rel=1e-7)


def measured(label, r32, r64, floor, expect_below=True):
    ref32 = R.relerr(r32, r64)
    print(f"{label}: ref32 {ref32:.2e} (floor {floor:.0e})")
    assert ref32 > 0
    assert (3 * ref32 < floor) == expect_below, (label, ref32)
    return ref32


@pytest.mark.parametrize("C", LN_C)
def test_ref32_of_the_layernorm_families(C):
    """Forward statistics and the backward from float32 statistics, on the draws of the GPU tests."""
    rows = 4099
    x, gamma, beta, gy, res = R.ln_inputs(rows, C, rows + C, special_rows=True)
    y64, m64, r64 = R.ln_fwd(x, gamma, beta, 1e-5, torch.float64)
    y32, m32, r32 = R.ln_fwd(x, gamma, beta, 1e-5, torch.float32)
    measured("ln_fwd mean", m32, m64, R.FLOOR)
    measured("ln_fwd rstd", r32, r64, R.FLOOR)
    assert 0 < 3 * float((y32.double() - y64).abs().max()) < 2e-4        # e32 of the bf16 bar: far below 2^-8 of O(1)
    x, gamma, beta, gy, res = R.ln_inputs(rows, C, rows + C)
    _, m32, r32 = R.ln_fwd(x, gamma, beta, 1e-5, torch.float32)
    want = R.ln_bwd_autograd(x, gamma, gy, 1e-5, res)
    got = R.ln_bwd(x, gamma, m32, r32, gy, torch.float32, res)
    measured("ln_bwd gx", got[0], want[0], R.FLOOR)
    measured("ln_bwd ggamma", got[1], want[1], R.REDUCTION_FLOOR)
    measured("ln_bwd gbeta", got[2], want[2], R.REDUCTION_FLOOR)


def test_ref32_of_the_elementwise_families():
    x = R.gelu_inputs(1_048_576 + 4099, 5)
    measured("gelu", R.gelu(x, torch.float32), R.gelu(x, torch.float64), R.FLOOR)
    d = torch.randn(x.shape, generator=torch.Generator().manual_seed(6))
    measured("gelu'", R.mul_dgelu(d, x, torch.float32), R.mul_dgelu(d, x, torch.float64), R.FLOOR)
    a, b = torch.randn(41472), torch.randn(41472)
    alpha = torch.tensor(0.37)
    measured("axpy", a + alpha * b, a.double() + alpha.double() * b.double(), R.FLOOR)
    v, r = torch.randn(4000), torch.randn(4000)
    measured("leaky + res", R.leaky(v) + r, R.leaky(v).double() + r.double(), R.FLOOR)
    rows = torch.randn(8200, 180) * torch.rand(8200)[:, None]
    measured("column sums", rows.sum(0), rows.double().sum(0), R.REDUCTION_FLOOR)
