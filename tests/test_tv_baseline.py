"""The TV baseline without a GPU: a float64 restatement of the algorithm models/tv.py documents (the discrete gradient and
its transpose, the primal-dual prox, proximal gradient descent) with its own closed forms, the host-side argument checks of
sei_tv_prox, and the model factory. tests/test_tv_baseline_gpu.py imports the restatement as the kernel's reference."""
import math

import pytest
import torch

TAU, RHO = 0.01, 1.99
SIGMA = 1.0 / (8.0 * TAU)


def nabla(x):
    """(.., H, W) -> (2, .., H, W): forward differences down and to the right, zero across the last row / column."""
    u = torch.zeros((2,) + tuple(x.shape), dtype=x.dtype)
    u[0][..., :-1, :] = x[..., 1:, :] - x[..., :-1, :]
    u[1][..., :, :-1] = x[..., :, 1:] - x[..., :, :-1]
    return u


def nabla_adjoint(u):
    """The exact transpose of nabla: (2, .., H, W) -> (.., H, W)."""
    x = torch.zeros(tuple(u.shape[1:]), dtype=u.dtype)
    x[..., :-1, :] -= u[0][..., :-1, :]
    x[..., 1:, :] += u[0][..., :-1, :]
    x[..., :, :-1] -= u[1][..., :, :-1]
    x[..., :, 1:] += u[1][..., :, :-1]
    return x


def tv_prox_ref(z, ths, state=None, iters=20):
    """`iters` iterations of the primal-dual loop in z's dtype; returns (x2, (x2, u2)). state None: x2 = z, u2 = 0."""
    x2, u2 = (z.clone(), torch.zeros((2,) + tuple(z.shape), dtype=z.dtype)) if state is None else state
    for _ in range(iters):
        x = (x2 - TAU * nabla_adjoint(u2) + TAU * z) / (1 + TAU)
        v = u2 + SIGMA * nabla(2 * x - x2)
        norm = torch.sqrt(v[0] * v[0] + v[1] * v[1])
        u = v / torch.clamp(norm / ths, min=1.0)
        x2 = x2 + RHO * (x - x2)
        u2 = u2 + RHO * (u - u2)
    return x2, (x2, u2)


def tv_pgd_ref(y, A, A_adjoint, lambd, stepsize=1.0, max_iter=300, n_it_max=20, early_stop=True):
    """Proximal gradient descent with the warm-started prox; returns (x, outer iterations run, last criterion)."""
    x = A_adjoint(y)
    state, crit, it = None, math.inf, -1
    for it in range(max_iter):
        x_prev = x
        z = x - stepsize * A_adjoint(A(x) - y)
        x, state = tv_prox_ref(z, lambd * stepsize, state, n_it_max)
        if it > 1:
            crit = float(torch.linalg.vector_norm(x_prev - x) / (torch.linalg.vector_norm(x) + 1e-6))
            if early_stop and crit < 1e-5:
                break
    return x, it + 1, crit


def blur_circ(x, k, transpose=False):
    """Direct circular convolution y[i, j] = sum_ab k[a, b] x[(i - a + kh // 2) mod H, (j - b + kw // 2) mod W] (BlurV2.A),
    or its transpose (the circular correlation)."""
    kh, kw = k.shape
    s = -1 if transpose else 1
    y = torch.zeros_like(x)
    for a in range(kh):
        for b in range(kw):
            y += k[a, b] * torch.roll(x, (s * (a - kh // 2), s * (b - kw // 2)), dims=(-2, -1))
    return y


def tv_value(x):
    u = nabla(x)
    return float(torch.sqrt(u[0] * u[0] + u[1] * u[1]).sum())


def objective(x, y, A, lambd):
    return 0.5 * float(((A(x) - y) ** 2).sum()) + lambd * tv_value(x)


def psnr(a, b):
    return 10.0 * math.log10(1.0 / float(((a - b) ** 2).mean()))


def gaussian_r2():
    import physics
    return physics.get_kernel("Gaussian_R2").double()


def piecewise_constant_case(hw=(40, 56), seed=0):
    """(clean, blurred + noisy) float64 (1, 3, H, W): two rectangles of level 0.8 / 0.4 on 0 plus 0.1 U[0, 1), blurred
    with Gaussian_R2, noise of sigma 0.05."""
    H, W = hw
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros((1, 3, H, W), dtype=torch.float64)
    x[..., H // 8: H // 2, W // 8: W // 2] = 0.8
    x[..., H // 3: 7 * H // 8, 3 * W // 5: 9 * W // 10] = 0.4
    x = x + 0.1 * torch.rand(x.shape, generator=g, dtype=torch.float64)
    y = blur_circ(x, gaussian_r2()) + 0.05 * torch.randn(x.shape, generator=g, dtype=torch.float64)
    return x, y


@pytest.mark.parametrize("H,W", [(5, 7), (1, 7), (7, 1), (1, 1)])
def test_nabla_adjoint_is_the_transpose(H, W):
    g = torch.Generator().manual_seed(H * 10 + W)
    x = torch.rand((2, H, W), generator=g, dtype=torch.float64)
    u = torch.rand((2, 2, H, W), generator=g, dtype=torch.float64)
    assert abs(float((nabla(x) * u).sum()) - float((x * nabla_adjoint(u)).sum())) < 1e-12
    d = nabla(x)
    assert float(d[0][..., -1, :].abs().max()) == 0.0 and float(d[1][..., :, -1].abs().max()) == 0.0    # Neumann


@pytest.mark.parametrize("a,b,ths", [(0.9, 0.1, 0.1), (0.55, 0.45, 0.1)])
def test_prox_of_two_pixels_reaches_the_closed_form(a, b, ths):
    """argmin 0.5 (x0 - a)^2 + 0.5 (x1 - b)^2 + ths |x1 - x0|: each value moves ths towards the other, or both meet."""
    if abs(a - b) > 2 * ths:
        want = [a - math.copysign(ths, a - b), b + math.copysign(ths, a - b)]
    else:
        want = [(a + b) / 2] * 2
    for z in (torch.tensor([[a, b]], dtype=torch.float64), torch.tensor([[a], [b]], dtype=torch.float64)):
        x, _ = tv_prox_ref(z, ths, iters=2000)
        err = float((x.flatten() - torch.tensor(want, dtype=torch.float64)).abs().max())
        assert err < 1e-9, err


def test_prox_splits_and_continues_from_its_state():
    g = torch.Generator().manual_seed(1)
    z = torch.rand((3, 9, 11), generator=g, dtype=torch.float64)
    whole, (x2, u2) = tv_prox_ref(z, 0.1, iters=20)
    part, state = tv_prox_ref(z, 0.1, iters=7)
    part, _ = tv_prox_ref(z, 0.1, state, iters=13)
    assert torch.equal(whole, part)
    assert float(u2[0][..., -1, :].abs().max()) == 0.0 and float(u2[1][..., :, -1].abs().max()) == 0.0


def test_blur_transpose_and_pgd_on_the_pinned_input():
    """The input of the GPU test: the restatement lowers the objective and gains at least 2 dB over the measurement."""
    k = gaussian_r2()
    g = torch.Generator().manual_seed(2)
    a = torch.rand((1, 2, 9, 15), generator=g, dtype=torch.float64)
    b = torch.rand((1, 2, 9, 15), generator=g, dtype=torch.float64)
    assert abs(float((blur_circ(a, k) * b).sum()) - float((a * blur_circ(b, k, transpose=True)).sum())) < 1e-12
    x, y = piecewise_constant_case()
    A, At = (lambda v: blur_circ(v, k)), (lambda v: blur_circ(v, k, transpose=True))
    for lambd in (0.02, 0.1):
        x_hat, ran, crit = tv_pgd_ref(y, A, At, lambd, max_iter=30, early_stop=False)
        assert ran == 30 and crit > 1e-5
        assert objective(x_hat, y, A, lambd) < objective(At(y), y, A, lambd)
        gain = psnr(x_hat, x) - psnr(y, x)
        print(f"lambd {lambd}: PSNR {psnr(y, x):.2f} dB -> {psnr(x_hat, x):.2f} dB (gain {gain:.2f} dB), criterion {crit:.1e}")
        assert gain >= 2.0


def test_pgd_early_stop_on_a_constant_measurement():
    k = gaussian_r2()
    y = torch.full((1, 3, 12, 16), 0.5, dtype=torch.float64)
    x_hat, ran, _ = tv_pgd_ref(y, lambda v: blur_circ(v, k), lambda v: blur_circ(v, k, transpose=True), 0.02)
    assert ran == 3 and float((x_hat - 0.5).abs().max()) < 1e-12


def test_entry_point_checks_its_arguments_on_the_host():
    import _native
    assert len(_native.SIGNATURES["sei_tv_prox"]) == 10 and len(_native.SIGNATURES["sei_tv_prox_ex"]) == 12
    assert len(_native.SIZE_QUERIES["sei_tv_prox_work_floats"]) == 3
    L = _native.lib()
    n = 2 * 8 * 8 * 4                                            # bytes of one copy of x2
    z, x2, u2, work = 4096, 4096 + n, 4096 + 2 * n, 4096 + 4 * n   # fake, disjoint, 4-byte aligned
    assert L.sei_tv_prox(None, None, None, 2, 8, 8, 0.1, 20, None, None) == 10001
    for args in ((None, x2, u2, work), (z, None, u2, work), (z, x2, None, work), (z, x2, u2, None)):
        assert L.sei_tv_prox(args[0], args[1], args[2], 2, 8, 8, 0.1, 20, args[3], None) == 10001
    for planes, H, W, iters in ((0, 8, 8, 20), (2, 0, 8, 20), (2, 8, -1, 20), (2, 8, 8, 0), (-1, 8, 8, 20)):
        assert L.sei_tv_prox(z, x2, u2, planes, H, W, 0.1, iters, work, None) == 10001
    for ths in (0.0, -0.1, math.nan):
        assert L.sei_tv_prox(z, x2, u2, 2, 8, 8, ths, 20, work, None) == 10001
    assert L.sei_tv_prox(z + 2, x2, u2, 2, 8, 8, 0.1, 20, work, None) == 10001                # off the 4-byte grid
    # aliasing: identical buffers, and partial overlaps of each pair (u2 is two copies long, work three)
    for a in ((z, z, u2, work), (z, x2, z, work), (z, x2, u2, z), (z, x2, x2, work), (z, x2, u2, x2), (z, x2, u2, u2),
              (z, x2, u2, u2 + n), (z, z + n - 4, u2, work), (z, x2, x2 + n - 4, work), (work + 3 * n - 4, x2, u2, work)):
        assert L.sei_tv_prox(a[0], a[1], a[2], 2, 8, 8, 0.1, 20, a[3], None) == 10001, a
    for tile, k in ((16, 5), (64, 3), (64, -1), (-32, 5), (128, 5), (64, 40)):                # not a built schedule
        assert L.sei_tv_prox_ex(z, x2, u2, 2, 8, 8, 0.1, 20, tile, k, work, None) == 10001
    assert L.sei_tv_prox(z, x2, u2, 1 << 15, (1 << 30) + 1, 8, 0.1, 20, work, None) == 10002
    # the workspace is one more copy of the state: x2 and the two planes of u2
    assert L.sei_tv_prox_work_floats(2, 8, 8) == 3 * 2 * 8 * 8
    assert L.sei_tv_prox_work_floats(3, 1356, 2040) == 3 * 3 * 1356 * 2040
    assert L.sei_tv_prox_work_floats(1, 1, 1) == 3
    for planes, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (1, (1 << 30) + 1, 8)):
        assert L.sei_tv_prox_work_floats(planes, H, W) == 0


def _args(*flags, **tv):
    """The common parser's arguments plus test.py's own --tv_lambd / --tv_max_iter (its defaults: None and 300)."""
    from settings import DefaultArgParser
    args = DefaultArgParser().parse_args(list(flags))
    args.tv_lambd, args.tv_max_iter = tv.get("tv_lambd"), tv.get("tv_max_iter", 300)
    return args


class StubPhysics:
    task = "deblurring"


def test_get_model_builds_the_tv_baseline():
    from models import get_model
    from models.tv import TV
    args = _args("--task", "deblurring", "--kernel", "Gaussian_R2", "--model_kind", "TV", tv_lambd=0.02)
    model = get_model(args, physics=StubPhysics(), device="cpu")
    tv = model.get_backbone()
    assert isinstance(tv, TV) and len(model.get_weights()) == 0 and list(model.parameters()) == []
    model.load_weights({})
    assert tv.lambd == 0.02 and tv.stepsize == 1.0 and tv.max_iter == 300 and tv.n_it_max == 20 and tv.early_stop
    assert get_model(_args("--model_kind", "TV", tv_lambd=0.1, tv_max_iter=7), physics=StubPhysics(),
                     device="cpu").get_backbone().max_iter == 7
    with pytest.raises(NotImplementedError, match="tv_lambd"):
        get_model(_args("--task", "deblurring", "--model_kind", "TV"), physics=StubPhysics(), device="cpu")


def test_the_baseline_refuses_cpu_tensors():
    import _native
    from models.tv import TV, tv_prox
    with pytest.raises(_native.NativeLibraryError):
        TV(StubPhysics(), lambd=0.02)(torch.rand(1, 3, 16, 16))
    with pytest.raises(_native.NativeLibraryError):
        tv_prox(torch.rand(3, 16, 16), 0.1)
