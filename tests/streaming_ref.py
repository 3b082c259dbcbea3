"""CPU references of the streaming kernels between the GEMMs (tests/test_streaming_swin_gpu.py and
tests/test_streaming_unet_loss_gpu.py compare the HIP kernels with them; tests/test_streaming_ref.py anchors them to
F.pad, to autograd and to the float32 format on the CPU first).

Plain torch on the CPU: nothing of the library under test is imported here. Three bars:

  exact    copies, one IEEE multiply / add / subtract, a round-to-nearest-even bf16 conversion: the same operation on the
           CPU in float32, compared bit for bit (`same_bits`: -0.0 and 0.0 differ).
  float32  (`hold32`) the float64 CPU reference, and the identical torch chain in float32; `ref32` is that chain's
           max-norm relative deviation from float64, and a kernel must sit within max(FLOOR, 3 * ref32) of float64
           relative to max |ref64| (the rule of tests/test_transform_edges_gpu.py). Column sums and LayerNorm parameter
           gradients take REDUCTION_FLOOR instead. The factor 3 is the margin for another summation order.
           (`hold32_on`: the same rule on a scale the caller names -- the sum of the absolute terms of a sum that
           cancels; tests/loss_reduction_ref.py.)
  bf16     (`hold_bf16`) per element |got - ref64| <= 2^-8 |ref64| + e32: the largest half-ulp of a round-to-nearest bf16
           value relative to it, and e32 = three times the float32 chain's max ABSOLUTE deviation on the same input.

For the inputs drawn here `ref32` stays below a third of the floors (tests/test_streaming_ref.py asserts it and
MEASURED_REF32 records the values), so the floors, not measured bars, are what the kernels are held to.
"""
import math

import torch
import torch.nn.functional as F

FLOOR = 5e-6
REDUCTION_FLOOR = 2e-5
BF16_HALF_ULP = 2.0 ** -8
MARGIN = 64                  # elements of sentinel on each side of an output (a multiple of 16 bytes for every type used)
SENTINEL = -7680.0           # exact in float32 and bfloat16 (-15 * 2^9), and nothing a kernel here computes

# ref32 of the families on the drawn inputs as tests/test_streaming_ref.py prints them (largest over its cases)
MEASURED_REF32 = {"ln_fwd mean": 8.3e-8, "ln_fwd rstd": 5.4e-8, "ln_bwd gx": 6.5e-7, "ln_bwd ggamma": 3.5e-7,
                  "ln_bwd gbeta": 2.0e-7, "column sums": 1.3e-7, "gelu": 3.0e-8, "gelu'": 1.6e-7, "axpy": 4.8e-8,
                  "leaky + res": 2.6e-8}


# ---------------------------------------------------------------------------------------------- bars
def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def bar(ref32, floor=FLOOR):
    return max(floor, 3 * ref32)


def hold32(label, got, r64, r32, floor=FLOOR):
    """got within max(floor, 3 * ref32) of r64, relative to max |r64|; prints and returns (deviation, ref32)."""
    assert bool(torch.isfinite(r64).all()), label
    ref32, err = relerr(r32, r64), relerr(got, r64)
    print(f"{label}: rel err {err:.2e}, ref32 {ref32:.2e}, bar {bar(ref32, floor):.2e}")
    assert err <= bar(ref32, floor), (label, err, ref32)
    return err, ref32


def hold32_abs(label, got, r64, r32, floor=FLOOR):
    """The same rule in absolute terms (results that are O(1) or vanish)."""
    got, r64, r32 = got.detach().cpu().double(), r64.double(), r32.double()
    ref32, err = float((r32 - r64).abs().max()), float((got - r64).abs().max())
    print(f"{label}: abs err {err:.2e}, ref32 {ref32:.2e}, bar {bar(ref32, floor):.2e}")
    assert err <= bar(ref32, floor), (label, err, ref32)
    return err, ref32


def hold32_on(label, got, r64, r32, scale, floor=FLOOR):
    """The same rule on a given scale: |got - r64| <= max(floor, 3 * ref32) * scale, ref32 = |r32 - r64| / scale. For a sum
    whose terms cancel, `scale` is the float64 sum of the absolute terms: the size of what the kernel added up, where
    max |r64| would be the size of what the inputs left over. Prints and returns (deviation, ref32), both on that scale."""
    got, r64, r32 = got.detach().cpu().double(), r64.double(), r32.double()
    scale = float(scale)
    assert got.shape == r64.shape and bool(torch.isfinite(r64).all()) and scale >= 0, label
    scale = max(scale, 1e-300)
    ref32, err = float((r32 - r64).abs().max()) / scale, float((got - r64).abs().max()) / scale
    print(f"{label}: err {err:.2e} of the scale {scale:.3e}, ref32 {ref32:.2e}, bar {bar(ref32, floor):.2e}")
    assert err <= bar(ref32, floor), (label, err, ref32)
    return err, ref32


def hold_bf16(label, got, r64, r32):
    """bf16 results of float32 arithmetic, per element; prints and returns (worst excess over 2^-8 |ref64|, e32)."""
    got, r64 = got.detach().cpu().double(), r64.double()
    assert got.shape == r64.shape and bool(torch.isfinite(r64).all()), label
    e32 = 3 * float((r32.double() - r64).abs().max())
    excess = float(((got - r64).abs() - BF16_HALF_ULP * r64.abs()).max())
    print(f"{label}: worst |got - ref64| - 2^-8 |ref64| {excess:.2e}, e32 {e32:.2e}")
    assert excess <= e32, (label, excess, e32)
    return excess, e32


def same_bits(a, b):
    """Equal shapes, types and bit patterns (NaN-free data; -0.0 is not 0.0)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    as_int = {8: torch.int64, 4: torch.int32, 2: torch.int16}[a.element_size()]
    return torch.equal(a.view(as_int), b.view(as_int))


# ---------------------------------------------------------------------------------------------- buffers
class Guarded:
    """An output of `shape` inside one allocation with MARGIN sentinel elements before and after it. The output proper is
    prefilled with the sentinel too, so a zero found in it was written by the kernel. Only values the test owns are
    looked at: nothing outside the allocation is touched."""

    def __init__(self, shape, dtype=torch.float32, device="cuda", fill=SENTINEL):
        shape = tuple(shape) if isinstance(shape, (tuple, list, torch.Size)) else (int(shape),)
        n = math.prod(shape)
        self.full = torch.full((n + 2 * MARGIN,), fill, dtype=dtype, device=device)
        self.view = self.full[MARGIN:MARGIN + n].view(shape)
        self.fill = fill

    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        lo, hi = self.full[:MARGIN].cpu(), self.full[-MARGIN:].cpu()
        return bool((lo == self.fill).all()) and bool((hi == self.fill).all())


def nan_tailed(t, device="cuda"):
    """A copy of `t` on `device` followed by MARGIN NaNs in the same allocation: what a kernel must not read. (An index
    map's tail holds -1, the hole: an index read from there must not send a wrong kernel outside the source.)"""
    flat = torch.full((t.numel() + MARGIN,), float("nan") if t.is_floating_point() else -1, dtype=t.dtype, device=device)
    flat[:t.numel()] = t.reshape(-1).to(device)
    return flat[:t.numel()].view(t.shape)


def nan_framed(t, lead, device="cuda"):
    """nan_tailed with `lead` NaNs in front as well: a contiguous copy of `t` that starts `lead` elements into its
    allocation (lead = 1: 4 bytes off the 16-byte grid for float32)."""
    flat = torch.full((lead + t.numel() + MARGIN,), float("nan"), dtype=t.dtype, device=device)
    flat[lead:lead + t.numel()] = t.reshape(-1).to(device)
    return flat[lead:lead + t.numel()].view(t.shape)


# ---------------------------------------------------------------------------------------------- padded grid
def padded_grid(x, guard, Cp=None, ones_col=False):
    """(B, H, W, C) -> (guard + B (H + 2) (W + 2) + guard, Cp) rows: a zero border around every image, `guard` zero rows
    before and after, channels C .. Cp - 1 zero; ones_col: channel C is 1 in EVERY row (border and guard rows too)."""
    B, H, W, C = x.shape
    Cp = C if Cp is None else Cp
    assert Cp >= C and (not ones_col or Cp > C)
    grid = torch.zeros((B, H + 2, W + 2, Cp), dtype=x.dtype)
    grid[:, 1:H + 1, 1:W + 1, :C] = x
    rows = torch.zeros((2 * guard + B * (H + 2) * (W + 2), Cp), dtype=x.dtype)
    rows[guard:guard + B * (H + 2) * (W + 2)] = grid.view(-1, Cp)
    if ones_col:
        rows[:, C] = 1
    return rows


def leaky(v):
    """LeakyReLU(0.01) as one float32 multiply on the not-positive side (0.0 and -0.0 are not > 0)."""
    return torch.where(v > 0, v, v * torch.tensor(0.01, dtype=v.dtype))


def leaky_gate(gate, dtype=None):
    """The LeakyReLU derivative factor from the pre-activation `gate`: 1 where gate > 0, else 0.01."""
    dtype = dtype or gate.dtype
    return torch.where(gate > 0, torch.tensor(1.0, dtype=dtype), torch.tensor(0.01, dtype=dtype))


# ---------------------------------------------------------------------------------------------- LayerNorm
def exact_constant(C):
    """A value c whose constant row has the same float32 mean whichever way it is formed: C c is exact in any summation
    order, and both (C c) / C and (C c) * fl(1 / C) round to c. Then x - mean is exactly 0 and y = beta."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    for c in (3.0, 1.0, 5.0, 7.0, 1.5, 2.5, 0.75):
        total = f32(c) * f32(float(C))
        if float(total) == c * C and float(total / f32(float(C))) == c and float(total * (f32(1.0) / f32(float(C)))) == c:
            return c
    raise AssertionError(f"no exact constant for C = {C}")


def ln_inputs(rows, C, seed, special_rows=False):
    """x = randn * 2 + 0.5 (float32), gamma, beta, gy, res. special_rows (rows >= 3): the last row is constant (variance 0:
    rstd = 1 / sqrt(eps), y = beta) and the one before it has mean 100 and unit spread."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, C), generator=gen) * 2 + 0.5
    gamma, beta = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    gy, res = torch.randn((rows, C), generator=gen), torch.randn((rows, C), generator=gen)
    if special_rows and rows >= 3:
        x[rows - 1] = exact_constant(C)
        x[rows - 2] = 100 + torch.randn(C, generator=gen)
    return x, gamma, beta, gy, res


def ln_fwd(x, gamma, beta, eps, dtype):
    """(y, mean, rstd) of LayerNorm over the last axis, biased variance, in `dtype`."""
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    mean = x.mean(1)
    d = x - mean[:, None]
    rstd = ((d * d).mean(1) + eps).rsqrt()
    return d * rstd[:, None] * gamma + beta, mean, rstd


def ln_bwd(x, gamma, mean, rstd, gy, dtype, res=None):
    """(gx, ggamma, gbeta) of LayerNorm from given row statistics, in `dtype`; gx = LN'(gy) + res."""
    x, gamma, mean, rstd, gy = (t.to(dtype) for t in (x, gamma, mean, rstd, gy))
    xh = (x - mean[:, None]) * rstd[:, None]
    t = gy * gamma
    gx = rstd[:, None] * (t - t.mean(1, keepdim=True) - xh * (t * xh).mean(1, keepdim=True))
    if res is not None:
        gx = gx + res.to(dtype)
    return gx, (gy * xh).sum(0), gy.sum(0)


def ln_bwd_autograd(x, gamma, gy, eps, res=None):
    """The same three gradients from torch.autograd.grad of F.layer_norm in float64."""
    xr, gr = x.double().requires_grad_(True), gamma.double().requires_grad_(True)
    br = torch.zeros_like(gr).requires_grad_(True)
    y = F.layer_norm(xr, (x.shape[1],), gr, br, eps)
    gx, gg, gb = torch.autograd.grad(y, [xr, gr, br], gy.double())
    return (gx if res is None else gx + res.double()), gg, gb


# ---------------------------------------------------------------------------------------------- bf16 casts and splits
def scaled_cast(x, scale=None):
    """(float32 rows x * s[:, None], their bf16 rounding): the float32 product first, then round-to-nearest-even."""
    v = x if scale is None else x * scale[:, None]
    return v, v.bfloat16()


def split_planes(x):
    """hi = bf16(x), lo = bf16(x - float(hi)): the subtraction is exact in float32 (it cancels the leading bits)."""
    hi = x.bfloat16()
    return hi, (x - hi.float()).bfloat16()


def split_inputs(n, seed):
    """n float32 values with magnitudes across 2^-20 .. 2^20; the first elements (as many as fit) are exact bf16 values
    (remainder 0) and bf16 ties (the 8th mantissa bit set and nothing below it, on even and odd neighbours)."""
    gen = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.rand(n, generator=gen) * 40 - 20)
    x = mag * (1 + torch.rand(n, generator=gen)) * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    exact = torch.tensor([1.0, -2.5, 2.0 ** -20, 2.0 ** 20, 0.0, -0.0, 1.0078125, 3.0 * 2.0 ** -19])
    tie_bits = torch.tensor([0x3F808000, 0x3F818000, 0xBF808000 - (1 << 32), 0x497F8000, 0x35808000, 0x35818000],
                            dtype=torch.int64).to(torch.int32)
    planted = torch.cat([exact, tie_bits.view(torch.float32)])[:n]
    x[:planted.numel()] = planted
    return x


# ---------------------------------------------------------------------------------------------- maps and ranges
def index_map(n, n_src, seed, holes=0.1):
    """n int32 indices into n_src >= n elements, every one used at most once, about `holes` of them replaced by -1."""
    gen = torch.Generator().manual_seed(seed)
    m = torch.randperm(n_src, generator=gen)[:n].to(torch.int32)
    m[torch.rand(n, generator=gen) < holes] = -1
    return m


def pack_ref(src, m):
    """dst[i] = src[m[i]], 0 in the holes."""
    return torch.where(m >= 0, src[m.clamp(min=0).long()], torch.zeros((), dtype=src.dtype))


def unpack_add_ref(src, m, dst):
    """dst[m[i]] += src[i] outside the holes (one float32 add per touched element), every other element untouched."""
    out, valid = dst.clone(), m >= 0
    out[m[valid].long()] += src[valid]
    return out


def zero_ranges_mask(n, pairs):
    """True at the elements of a buffer of n that the (offset, length) pairs name."""
    mask = torch.zeros(n, dtype=torch.bool)
    for off, length in pairs:
        assert 0 <= off and off + length <= n
        mask[off:off + length] = True
    return mask


# ---------------------------------------------------------------------------------------------- GELU
GELU_FIXED = (0.0, -0.0, 1e-30, -1e-30, 0.5, -0.5, 6.0, -6.0, 13.0, -13.0, 40.0, -40.0)


def gelu_inputs(n, seed):
    """randn * 3 with the fixed points in front (as many as fit)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=gen) * 3
    k = min(n, len(GELU_FIXED))
    x[:k] = torch.tensor(GELU_FIXED[:k])
    return x


def gelu(x, dtype):
    return F.gelu(x.to(dtype))


def mul_dgelu(d, h, dtype):
    """d * gelu'(h) as torch.autograd.grad of F.gelu with the cotangent d."""
    hr = h.to(dtype).requires_grad_(True)
    (g,) = torch.autograd.grad(F.gelu(hr), hr, d.to(dtype))
    return g
