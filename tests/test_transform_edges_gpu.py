"""The equivariant transforms where the U-Net's own 48 x 48 crops never take them: the scale transform's backward on
rectangular, odd, tiny and 1-pixel images and at rates outside the table (reflections of several spans), the kernel
with a sampled image of another size than the grid (Hi != H: the antialiased variant) alone and behind the antialias
pre-filter, the `normal` kind's backward, the rotation above 1024 planes and on single rows and columns, and the host
side refusals of the four entry points.

Reference for sections 1 to 4: the oracle's torch path (or F.grid_sample on the oracle's grid) on the CPU in float64,
torch.autograd.grad for the backward. The bar is the rule of tests/test_physics_gpu.py::test_scale_transform_vs_golden:
the identical CPU chain is run in float32 as well, its max-norm relative deviation from the float64 run is `ref32`, and
the HIP result must sit within max(5e-6, 3 * ref32) of the float64 run. Float32 sampling positions carry about
W * 2^-24 pixels of rounding in torch's own path too, so the bar is the reference's own float32 deviation with a factor
3 of margin, never a figure taken from the code under test. The backward accumulates with float atomicAdd: no test asks
two runs for equal bits.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import closed_form as cf
from oracle import torch_path as tp

pytestmark = pytest.mark.gpu
FLOOR = 5e-6


def relerr(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def draws(x_shape, g_shape, seed):
    """x = rand, cotangent g = randn, centres 2 * rand - 1 with image 0's pinned to the corner (-1, 1): CPU float32."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(x_shape, generator=gen)
    g = torch.randn(g_shape, generator=gen)
    center = 2 * torch.rand((x_shape[0], 2), generator=gen) - 1
    center[0, 0], center[0, 1] = -1.0, 1.0
    return x, g, center.view(-1, 1, 1, 2)


def cpu_chain(fn, x, g, dtype):
    """(fn(x), its vector-Jacobian product with g) on the CPU in `dtype`; fn takes (x, dtype)."""
    xr = x.detach().to(dtype, copy=True).requires_grad_(True)
    y = fn(xr, dtype)
    (gx,) = torch.autograd.grad(y, xr, g.to(dtype))
    return y.detach(), gx


def gpu_chain(fn, x, g):
    xd = x.cuda().requires_grad_(True)
    y = fn(xd)
    (gx,) = torch.autograd.grad(y, xd, g.cuda())
    torch.cuda.synchronize()
    return y.detach(), gx


def hold_to_float64(label, gpu, ref_fn, x, g):
    """Forward and backward of `gpu` = (y, gx) against the float64 CPU chain, each within max(5e-6, 3 * ref32)."""
    y64, gx64 = cpu_chain(ref_fn, x, g, torch.float64)
    y32, gx32 = cpu_chain(ref_fn, x, g, torch.float32)
    assert bool(torch.isfinite(y64).all()) and bool(torch.isfinite(gx64).all())
    assert gpu[0].shape == y64.shape and gpu[1].shape == gx64.shape == x.shape
    for what, got, r64, r32 in (("fwd", gpu[0], y64, y32), ("bwd", gpu[1], gx64, gx32)):
        ref32 = relerr(r32, r64)
        err = relerr(got, r64)
        print(f"{label} {what}: rel err {err:.2e}, ref32 {ref32:.2e}, bar {max(FLOOR, 3 * ref32):.2e}")
        assert err < max(FLOOR, 3 * ref32), (label, what, err, ref32)


def hold_transpose(label, x, g, y, gx):
    """<T x, g> = <x, T^T g> on the GPU results: float32 products summed in float64, the bar of
    tests/test_loss_gpu.py::test_rotate_transform_vs_oracle."""
    lhs = float((y.double().cpu() * g.double()).sum())
    rhs = float((gx.detach().double().cpu() * x.double()).sum())
    print(f"{label} transpose: <Tx, g> {lhs:.9g}, <x, T'g> {rhs:.9g}, diff {abs(lhs - rhs):.2e}")
    assert abs(lhs - rhs) <= 1e-6 * max(1.0, abs(lhs)), (label, lhs, rhs)


# ------------------------------------------------------------------ 1. padded scale transform, forward and backward
PADDED = [
    ((3, 2, 24, 40), (.75, .5, .75)),       # W > H: the p / H re-indexing of the reference's view() in the backward
    ((2, 3, 40, 24), (.5, .75)),            # H > W
    ((2, 1, 37, 53), (.75, .5)),            # odd extents, B*H*W no multiple of 256, one channel
    ((5, 2, 7, 9), (.5, .75, .5, .75, .5)),     # five images inside two workgroups: b changes within a wavefront
    ((2, 2, 1, 9), (.5, .75)),              # reflect_clip's n == 1 branch; (Hi - 1) == 0
    ((2, 2, 9, 1), (.5, .75)),
    ((2, 2, 2, 3), (.5, .75)),              # spans 1 and 2: every outside tap reflects several times
    ((1, 1, 1, 1), (.5,)),                  # the degenerate image
    ((3, 2, 4, 4), (.1, .3, 1.7)),          # rates outside the table: many flips, and a zoom-in
    ((2, 3, 5, 6), (1.0, 2.5)),             # rate 1 is not the identity on this grid; a zoom-in
]


@pytest.mark.parametrize("shape,rates", PADDED, ids=lambda v: "x".join(str(k) for k in v))
def test_padded_scale_transform_fwd_bwd_vs_float64(shape, rates):
    """padded_downsampling_transform (sei_scale_resample_fwd / _bwd with Hi == H) against oracle.scale_transform in
    float64, output and gradient, one rate per image; and the transpose relation between the two kernels."""
    import transforms
    assert len(rates) == shape[0]
    x, g, center = draws(shape, shape, seed=41)
    rate = torch.tensor(rates, dtype=torch.float32)
    y, gx = gpu_chain(lambda xd: transforms.padded_downsampling_transform(xd, rate.cuda(), center.cuda(), "bicubic",
                                                                          "reflection", False), x, g)
    hold_to_float64(f"padded {shape} {rates}", (y, gx),
                    lambda xr, dt: tp.scale_transform(xr, rate.to(dt), center.to(dt)), x, g)
    hold_transpose(f"padded {shape} {rates}", x, g, y, gx)


# ------------------------------------------------------------------ 2. the kernel with Hi != H, without the pre-filter
SAMPLED = [((27, 39), (37, 53)), ((10, 15), (21, 30)), ((6, 8), (9, 11)), ((1, 3), (2, 5)),
           ((40, 12), (20, 24))]            # the last: taller and narrower than the grid


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("in_hw,out_hw", SAMPLED, ids=lambda v: "x".join(str(k) for k in v))
def test_scale_resample_kernel_on_another_size_than_the_grid(in_hw, out_hw, C):
    """_ScaleResample on a random (Hi, Wi) image sampled on the (H, W) grid -- the kernel of the antialiased variant,
    isolated -- against float64 F.grid_sample on oracle.scale_grid; the gradient has the sampled image's shape."""
    import transforms
    B = 2
    x, g, center = draws((B, C) + in_hw, (B, C) + out_hw, seed=43)
    rate = torch.tensor([0.75, 0.5])

    def ref(xr, dt):
        grid = tp.scale_grid((B, C) + out_hw, rate.to(dt), center.to(dt), dt)
        return F.grid_sample(xr, grid, mode="bicubic", padding_mode="reflection", align_corners=True)

    y, gx = gpu_chain(lambda xd: transforms._ScaleResample.apply(xd, rate.cuda(), center.cuda(), out_hw), x, g)
    assert y.shape == (B, C) + out_hw and gx.shape == (B, C) + in_hw
    hold_to_float64(f"sampled {in_hw}->{out_hw} C={C}", (y, gx), ref, x, g)


# ------------------------------------------------------------------ 3. antialiased padded variant, the whole chain
ANTIALIASED = [((2, 3, 48, 48), 0.75, (36, 36)), ((2, 2, 37, 53), 0.75, (27, 39)), ((2, 2, 37, 53), 0.5, (18, 26)),
               ((1, 2, 21, 30), 0.5, (10, 15)), ((2, 1, 9, 11), 0.75, (6, 8))]


@pytest.mark.parametrize("shape,rate,inner", ANTIALIASED, ids=lambda v: str(v).replace(" ", ""))
def test_antialiased_padded_transform_fwd_bwd_vs_float64(shape, rate, inner):
    """padded_downsampling_transform(antialiased=True) -- the banded antialias resize to floor(H rate) x floor(W rate),
    then the kernel with Hi != H, and on the way back that kernel's backward chained into the resize's transpose --
    against oracle.scale_transform(antialias=True) in float64. One rate for the batch, as the reference's stack needs."""
    import transforms
    x, g, center = draws(shape, shape, seed=47)
    rates = torch.full((shape[0],), rate)
    assert tuple(F.interpolate(x[:1], scale_factor=rate, mode="bicubic", antialias=True).shape[-2:]) == inner
    gpu = gpu_chain(lambda xd: transforms.padded_downsampling_transform(xd, rates.cuda(), center.cuda(), "bicubic",
                                                                        "reflection", True), x, g)
    hold_to_float64(f"antialiased {shape} {rate}", gpu,
                    lambda xr, dt: tp.scale_transform(xr, rates.to(dt), center.to(dt), antialias=True), x, g)


# ------------------------------------------------------------------ 4. the `normal` kind's backward
@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("rate", [0.75, 0.5])
@pytest.mark.parametrize("shape", [(2, 3, 24, 24), (2, 2, 37, 53), (1, 1, 9, 11)])
def test_normal_transform_fwd_bwd_vs_float64(shape, rate, aa):
    """normal_downsampling_transform (the banded resize and, backward, its transpose) against
    oracle.scale_transform_normal in float64, output and gradient."""
    import transforms
    out_hw = tuple(tp.scale_transform_normal(torch.zeros((1, 1) + shape[-2:]), rate, aa).shape[-2:])
    x, g, _ = draws(shape, shape[:2] + out_hw, seed=53)
    gpu = gpu_chain(lambda xd: transforms.normal_downsampling_transform(xd, rate, "bicubic", aa), x, g)
    hold_to_float64(f"normal {shape} {rate} aa={aa}", gpu, lambda xr, dt: tp.scale_transform_normal(xr, rate, aa), x, g)


# ------------------------------------------------------------------ 5. rotation at its extents
ROTATIONS = [
    ((1030, 1, 5, 7), (37.0, 90.0, 45.0)),      # 1030 planes > 1024: the c += gridDim.y loop
    ((1, 1, 1, 9), (37.0, 90.0, 45.0)),         # one row
    ((1, 1, 9, 1), (37.0, 90.0, 45.0)),         # one column
    ((1, 2, 2, 2), (37.0, 90.0)),               # (at 45 degrees every pixel of a 2 x 2 image sits on a rounding tie)
    ((1, 1, 16, 15), (37.0, 45.0)),             # even by odd (at 90 degrees every pixel sits on a tie)
]


@pytest.mark.parametrize("shape,angles", ROTATIONS, ids=lambda v: "x".join(str(int(k)) for k in v))
def test_rotate_transform_at_its_extents(shape, angles):
    """sei_rotate_nearest_fwd / _bwd, by the method of tests/test_loss_gpu.py::test_rotate_transform_vs_oracle: the output
    equals oracle.rotate_nearest wherever the source coordinate is further than 1e-4 from a rounding tie, the backward
    is the exact transpose of the forward, and where no pixel differs it is the CPU autograd gradient. At most 2 % of
    the pixels may be ties (asserted on the oracle first), so that the comparison is never empty."""
    import transforms
    gen = torch.Generator().manual_seed(21)
    x = torch.rand(shape, generator=gen)
    g = torch.randn(shape, generator=gen)
    planes = shape[0] * shape[1]
    t = transforms.Rotate()
    for angle in angles:
        margin = tp.rotate_source_margin(shape[-2:], angle)
        ties = float((margin <= 1e-4).double().mean())
        assert ties <= 0.02, (angle, ties)
        ref = tp.rotate_nearest(x, angle)
        xr = x.clone().requires_grad_(True)
        tp.rotate_nearest(xr, angle).backward(g)
        xd = x.cuda().requires_grad_(True)
        out = t(xd, params=[angle])
        assert out.shape == ref.shape
        differs = (out.detach().cpu() != ref).any(dim=0).any(dim=0)
        assert not bool((differs & (margin > 1e-4)).any()), angle
        out.backward(g.cuda())
        lhs = float((out.detach().double().cpu() * g.double()).sum())
        rhs = float((xd.grad.double().cpu() * x.double()).sum())
        print(f"rotate {shape} {angle}: ties {ties:.3f}, differing pixels {int(differs.sum())}, "
              f"transpose diff {abs(lhs - rhs):.2e} of {abs(lhs):.4g}")
        assert abs(lhs - rhs) <= 1e-6 * max(1.0, abs(lhs)), (angle, lhs, rhs)
        if not bool(differs.any()):
            assert torch.allclose(xd.grad.cpu(), xr.grad, atol=1e-6), angle
        if planes > 1024:
            # the planes that only the second trip of the loop writes, by themselves
            assert ties == 0.0 and not bool(differs.any()), angle
            tail_out = out.detach().cpu().reshape(planes, *shape[-2:])[1024:]
            tail_grad = xd.grad.cpu().reshape(planes, *shape[-2:])[1024:]
            assert tail_out.shape[0] == planes - 1024
            assert torch.equal(tail_out, ref.reshape(planes, *shape[-2:])[1024:]), angle
            assert torch.allclose(tail_grad, xr.grad.reshape(planes, *shape[-2:])[1024:], atol=1e-6), angle
            assert bool(tail_out.abs().sum() > 0) and bool(tail_grad.abs().sum() > 0), angle


# ------------------------------------------------------------------ 6. host-side argument checks
# Fake device pointers for calls that must be refused: never dereferenced, because a refused call launches nothing.
P0, P1, P2, P3 = 4096, 8192, 12288, 16384
BAD_ARG = 10001


@pytest.mark.parametrize("name", ["sei_scale_resample_fwd", "sei_scale_resample_bwd"])
def test_scale_resample_entry_points_refuse_bad_arguments(name):
    """x == y (gy == gx), a null operand and a zero extent are refused on the host with SEI_ERR_BAD_ARG, before any
    launch: every call below carries exactly one reason to be refused."""
    import _native
    fn = getattr(_native.lib(), name)
    sizes = dict(B=2, C=3, Hi=6, Wi=8, H=9, W=11)
    assert len(_native.SIGNATURES[name]) == 4 + len(sizes) + 1
    assert fn(P0, P0, P2, P3, *sizes.values(), None) == BAD_ARG, "aliased input and output"
    for k in range(4):
        ptrs = [P0, P1, P2, P3]
        ptrs[k] = None
        assert fn(*ptrs, *sizes.values(), None) == BAD_ARG, f"null pointer {k}"
    for key in sizes:
        for bad in (0, -1):
            assert fn(P0, P1, P2, P3, *dict(sizes, **{key: bad}).values(), None) == BAD_ARG, f"{key} = {bad}"


@pytest.mark.parametrize("name", ["sei_rotate_nearest_fwd", "sei_rotate_nearest_bwd"])
def test_rotate_entry_points_refuse_bad_arguments(name):
    """An image of 2^30 pixels or more (the kernels index a plane with an int), aliased or null operands and a zero
    extent are refused on the host with SEI_ERR_BAD_ARG, before any launch."""
    import _native
    fn = getattr(_native.lib(), name)
    theta = (0.0, -1.0, 1.0, 0.0)
    assert len(_native.SIGNATURES[name]) == 2 + 3 + 4 + 1
    for H, W in ((1 << 15, 1 << 15), (1 << 30, 1), (1, 1 << 30), (46341, 46341), (1 << 16, 1 << 16)):
        assert H * W >= 1 << 30
        assert fn(P0, P1, 1, H, W, *theta, None) == BAD_ARG, (H, W)
    assert fn(P0, P0, 1, 8, 8, *theta, None) == BAD_ARG
    assert fn(None, P1, 1, 8, 8, *theta, None) == BAD_ARG and fn(P0, None, 1, 8, 8, *theta, None) == BAD_ARG
    for planes, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 0)):
        assert fn(P0, P1, planes, H, W, *theta, None) == BAD_ARG, (planes, H, W)
