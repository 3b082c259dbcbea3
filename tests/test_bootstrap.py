"""CPU: the equivariant bootstrap's entry points exist and refuse bad arguments without a GPU, test.py takes its flags,
and the float64 reference of tests/bootstrap_ref.py is anchored: its zoom-out against F.grid_sample on the reference-order
grid where the two layouts agree (square extents), its pull-back against the image it started from.

Measured on the reference alone (printed by test_ref_pull_back_of_the_zoom_out_is_close_to_the_image, which says what the
bar is and where the composition lands): see its docstring.
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import bootstrap_ref as R

NEW_SYMBOLS = ("sei_boot_scale_fwd", "sei_boot_luma_diff", "sei_boot_luma_diff_work_floats", "sei_boot_pullback_accum")


def test_new_symbols_are_exported_and_bound():
    import _native
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name), name
        assert name in _native.SIGNATURES or name in _native.SIZE_QUERIES, name
    assert _native.SIGNATURES["sei_boot_scale_fwd"] == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    assert handle.sei_abi_version() == 12


def test_new_symbols_refuse_bad_arguments_without_a_gpu():
    import _native
    L = _native.lib()
    P = 4096                                             # a fake device pointer: a refused call launches nothing
    assert L.sei_boot_scale_fwd(None, None, None, None, 1, 3, 8, 8, None) == 10001
    assert L.sei_boot_scale_fwd(P, P + 4096, P, None, 1, 3, 8, 8, None) == 10001
    for bad in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1), (1, 3, 1 << 15, 1 << 15)):
        assert L.sei_boot_scale_fwd(P, 2 * P, P, P, *bad, None) == 10001, bad
    assert L.sei_boot_luma_diff(None, None, 1, 64, None, None, None, None) == 10001
    assert L.sei_boot_luma_diff(P, P, 1, 64, P, P, None, None) == 10001
    assert L.sei_boot_luma_diff(P, P, 0, 64, P, P, P, None) == 10001
    assert L.sei_boot_luma_diff(P, P, 1, 0, P, P, P, None) == 10001
    assert L.sei_boot_luma_diff(P, P, 65536, 64, P, P, P, None) == 10001
    assert L.sei_boot_luma_diff(P, P, 1, 1 << 30, P, P, P, None) == 10001
    assert L.sei_boot_pullback_accum(None, None, None, 1, 8, 8, None, 0, None) == 10001
    assert L.sei_boot_pullback_accum(P, P, P, 1, 8, 8, None, 0, None) == 10001
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 1 << 15, 1 << 15)):
        assert L.sei_boot_pullback_accum(P, P, P, *bad, 2 * P, 0, None) == 10001, bad
    # the size query: 0 where the entry point refuses, a function of the pixel count alone per image otherwise
    q = L.sei_boot_luma_diff_work_floats
    assert q(0, 64) == 0 and q(1, 0) == 0 and q(65536, 64) == 0 and q(1, 1 << 30) == 0
    assert q(1, 1) == 1 and q(3, 45) == 3 and q(1, 257) == 2 and q(4, 257) == 8 and q(2, 1 << 20) == 2 * 256


def load_test_py():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("sei_test_driver", os.path.join(root, "test.py"))
    driver = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(driver)
    return driver


def test_test_py_takes_the_bootstrap_flags(capsys):
    test_py = load_test_py()
    args = test_py.parse_args(["--task", "deblurring"])
    assert (args.bootstrap, args.bootstrap_batch, args.bootstrap_maps) == (0, 8, False)
    args = test_py.parse_args(["--task", "deblurring", "--bootstrap", "16", "--bootstrap_batch", "2", "--bootstrap_maps",
                               "--out_dir", "somewhere"])
    assert (args.bootstrap, args.bootstrap_batch, args.bootstrap_maps) == (16, 2, True)
    with pytest.raises(SystemExit):
        test_py.parse_args(["--task", "deblurring", "--bootstrap", "4", "--bootstrap_maps"])
    assert "--out_dir" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        test_py.parse_args(["--task", "deblurring", "--bootstrap", "4", "--bootstrap_batch", "0"])


def test_bootstrap_refuses_cpu_tensors_and_bad_arguments():
    import _native
    import physics
    from bootstrap import EquivariantBootstrap
    op = physics.BlurV2(kernel=physics.get_kernel("Gaussian_R2")[None, None])
    boot = EquivariantBootstrap(op, lambda v: v, samples=2)
    with pytest.raises(_native.NativeLibraryError):
        boot(torch.rand(3, 16, 16))
    with pytest.raises(TypeError):                       # the padded scale transform is the only one: no way to name another
        EquivariantBootstrap(op, lambda v: v, samples=2, transform="shift")
    with pytest.raises(ValueError):
        EquivariantBootstrap(op, lambda v: v, samples=2, rates=(0.75, 1.5))
    with pytest.raises(ValueError):
        EquivariantBootstrap(op, lambda v: v, samples=0)


def reference_order_grid(B, h, w, rate, center):
    """The (w, h) meshgrid viewed as (h, w) of the reference's transform, restated: u over w, v over h, meshgrid 'ij' of
    (u, v), the pair (V, U) stacked, and the (w, h, 2) result VIEWED as (h, w, 2)."""
    u = 2 / w * torch.arange(w, dtype=torch.float64) - 1
    v = 2 / h * torch.arange(h, dtype=torch.float64) - 1
    U, V = torch.meshgrid(u, v, indexing="ij")
    grid = torch.stack([V, U], dim=-1).reshape(1, h, w, 2).repeat(B, 1, 1, 1)
    c = center.double().view(B, 1, 1, 2)
    return 1 / rate.double().view(B, 1, 1, 1) * (grid - c) + c


def draws(B, seed):
    gen = torch.Generator().manual_seed(seed)
    rate = torch.tensor([0.75, 0.5])[torch.randint(0, 2, (B,), generator=gen)]
    return rate, 2 * torch.rand((B, 2), generator=gen) - 1


@pytest.mark.parametrize("n", [1, 8, 13, 48])
def test_ref_zoom_out_equals_grid_sample_on_the_reference_order_grid_where_square(n):
    rate, center = draws(4, n)
    x = torch.rand((3, n, n), generator=torch.Generator().manual_seed(n), dtype=torch.float64)
    want = F.grid_sample(x[None].expand(4, 3, n, n), reference_order_grid(4, n, n, rate, center), mode="bicubic",
                         padding_mode="reflection", align_corners=True)
    assert torch.equal(R.zoom_out(x, rate, center), want)


def test_ref_layouts_part_where_not_square():
    """On 5 x 9 the reference-order grid is a different grid (what the new kernel does not inherit): the reference's own
    check that the square agreement above is not vacuous."""
    rate, center = torch.tensor([0.5]), torch.zeros(1, 2)
    assert not torch.allclose(R.forward_grid(5, 9, rate, center), reference_order_grid(1, 5, 9, rate, center))
    g = R.forward_grid(5, 9, rate, center)[0]
    assert torch.equal(g[:, :, 0], g[:1, :, 0].expand(5, 9)) and torch.equal(g[:, :, 1], g[:, :1, 1].expand(5, 9))


PERIODS = ((16, 24), (32, 16), (20, 20))


def smooth_image(i, j):
    """Three planes of low-frequency waves in [0, 1] at the (fractional) rows i and columns j: shortest period 16 pixels."""
    return torch.stack([0.5 + 0.25 * torch.cos(2 * math.pi * (i / p + 0.1 * k)) * torch.cos(2 * math.pi * (j / q - 0.2 * k))
                        + 0.2 * torch.sin(2 * math.pi * (i + j) / (p + q)) for k, (p, q) in enumerate(PERIODS)])


# max |T^+ T x - x at the landing position| on the interior, as this test printed it on the float64 reference
RECORDED_PULLBACK_ERROR = {(0.75, 0.0, 0.0): 1.47e-2, (0.5, 0.0, 0.0): 2.01e-2, (0.5, 0.3, -0.2): 1.95e-2}


@pytest.mark.parametrize("rate,cx,cy", [(0.75, 0.0, 0.0), (0.5, 0.0, 0.0), (0.5, 0.3, -0.2)])
def test_ref_pull_back_of_the_zoom_out_is_close_to_the_image(rate, cx, cy):
    """T^+ T x against x for a smooth x, up to the error of two bicubic interpolations.

    Where the composition lands: the grid of a pixel is g(j) = (2 / W) j - 1, but align_corners=True reads a grid value g
    at the pixel (g + 1) (W - 1) / 2, so even rate 1 samples pixel j at k j, k = (W - 1) / W (the reference's convention,
    kept by the loss and by this transform). Composing T^+ after T gives, per axis, the position
        k^2 j + (c + 1) (k / 2) (1 - 1 / rate),
    up to two pixels from j at the far border. The pull-back is held to x AT THAT POSITION (x is analytic here); the
    deviation from x at j itself is printed: it is the displacement, not interpolation error, and one of the reasons the
    error map is a qualitative picture.

    "Close" is the error of the two bicubic interpolations, measured on this reference and recorded above (1.5e-2 and
    2.0e-2 of an image of range 0.9, shortest period 16 pixels); the bar is three times the recorded figure. Against x at
    the pixel itself the deviation is 0.25 to 0.31, and the test asserts that it is beyond the bar: the displacement is
    pinned, not only printed."""
    H, W = 48, 40
    i = torch.arange(H, dtype=torch.float64)[:, None].expand(H, W)
    j = torch.arange(W, dtype=torch.float64)[None, :].expand(H, W)
    x = smooth_image(i, j)
    r, c = torch.tensor([rate]), torch.tensor([[cx, cy]], dtype=torch.float64)
    a = R.zoom_out(x, r, c)[0]
    back = torch.stack([R.pull_back(a[k][None], r, c)[0] for k in range(3)])
    kw, kh = (W - 1) / W, (H - 1) / H
    landed = smooth_image(kh * kh * i + (cy + 1) * (kh / 2) * (1 - 1 / rate), kw * kw * j + (cx + 1) * (kw / 2) * (1 - 1 / rate))
    # T x is x only where T's sample points lie inside the image; T^+ reads it there and two taps around: stay clear of the
    # frame that reflection fills
    m = 6
    inner = (slice(None), slice(m, H - m), slice(m, W - m))
    err = float((back - landed)[inner].abs().max())
    naive = float((back - x)[inner].abs().max())
    bar = 3 * RECORDED_PULLBACK_ERROR[(rate, cx, cy)]
    print(f"pull-back of the zoom-out at rate {rate} about ({cx}, {cy}): max err {err:.2e} (bar {bar:.2e}); against the "
          f"image at the pixel itself {naive:.2e}")
    assert err <= bar
    assert naive > bar


def test_ref_quantize_is_the_float32_chain():
    k = torch.arange(255, dtype=torch.float64)
    ties = ((k + 0.5) / 255).float()
    x = torch.cat([ties, torch.nextafter(ties, torch.tensor(2.0)), torch.nextafter(ties, torch.tensor(-1.0)),
                   torch.tensor([-0.3, 1.7, 0.0, 1.0])])
    q = R.quantize(x.double())
    assert q.dtype == torch.float64 and torch.equal(q.float(), ((x * 255.0).round() / 255.0).clamp(0.0, 1.0))


def test_ref_closed_form_of_the_constant_image():
    """The GPU test's closed form on the reference itself: x_hat = 0.4 (a zoom-out of a constant is the constant, the blur
    of a constant too), noise level 5, identity model: d = Y(q(0.4)) - Y(q(0.4 + sigma n)), whose mean square is
    ((sigma 255)^2 + 1/12) / 255^2 (0.299^2 + 0.587^2 + 0.114^2) up to the quantisation of a Gaussian at this width."""
    N, H, W = 16, 48, 40
    value = (25 + 1 / 12) / 255 ** 2 * sum(c * c for c in R.LUMA)
    assert abs(value - 1.7242e-4) < 1e-8
    gen = torch.Generator().manual_seed(0)
    rate, center = draws(N, 3)
    noise = torch.randn((N, 3, H, W), generator=gen, dtype=torch.float64)
    out = R.bootstrap(torch.full((3, H, W), 0.4, dtype=torch.float64), rate, center, noise, lambda v: v, 5 / 255)
    se = value * math.sqrt(2 / (N * H * W))
    assert abs(float(out["mse"].mean()) - value) <= 5 * se
