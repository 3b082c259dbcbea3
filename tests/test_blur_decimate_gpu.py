"""physics.BlurDownsampling on the GPU: A and A_adjoint against float64 (tests/blur_decimate_ref.py), the two composition
identities against the existing Blur / BlurV2, the tile and wrap edges of sei_blur_decimate, the dot test, run-to-run bits,
autograd and capture, and the operator inside the losses, train.py and test.py.

The bars are the project's own: max-norm relative 2e-6 (tests/test_physics_gpu.py), dot test 1e-5, loss 1e-4 and gradient
norm 1e-3 (tests/test_blur_padding_gpu.py).

On tile halving: the forward tile is 16 x 32 MEASUREMENT pixels cut to the measurement's extents, under 64 KiB of LDS. The
63x3 taps at rate 4 on 40x72 of the edge list stage 99 x 72 floats (29 KB) for their single 10 x 18 tile, which fits: that
case covers the tallest footprint per output row, not the halving. `63x63 at rate 8` below is the case that halves (16 x 32
-> 1 x 16 at 64 x 256)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from blur_decimate_ref import rand_kernel, reference64, relerr

pytestmark = pytest.mark.gpu
TOL = 2e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PADDINGS = ("circular", "replicate", "reflect")


def operator(k, rate, padding, phase=0, v2=True):
    import physics
    return physics.BlurDownsampling(filter=k[None, None].cuda(), rate=rate, padding=padding, phase=phase, v2=v2)


def blur_of(k, padding, v2=True):
    """The operator --task deblurring builds from the same kernel, --blur_padding and --physics_v2."""
    import physics
    if v2 and padding == "circular":
        return physics.BlurV2(kernel=k[None, None].cuda())
    return physics.Blur(filter=k[None, None].cuda(), padding=padding, device="cuda")


def transpose_to(op, g, hw):
    """The exact transpose of A on images of extents `hw` (A_adjoint itself assumes (rate h, rate w))."""
    from physics._ops import apply_linear
    return apply_linear(op._op, g.contiguous(), transpose=True, out_hw=hw)


def rule_of(padding, v2):
    return "v2" if padding == "circular" and v2 else "legacy"


def kernel_named(name):
    import physics
    return physics.get_kernel("Gaussian_R1") if name == "Gaussian_R1" else rand_kernel(5, 4, 3)


BOUNDARIES = [("circular", True), ("circular", False), ("replicate", True), ("reflect", True)]


@pytest.fixture(scope="module")
def image():
    return torch.rand((2, 3, 37, 50), generator=torch.Generator().manual_seed(1)).cuda()


# ------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("padding,v2", BOUNDARIES, ids=[f"{p}-{'v2' if v else 'legacy'}" for p, v in BOUNDARIES])
@pytest.mark.parametrize("name", ["rand5x4", "Gaussian_R1"])
@pytest.mark.parametrize("rate", [2, 3, 4])
def test_vs_float64(image, rate, name, padding, v2):
    k = kernel_named(name)
    for phase in (0, rate - 1):
        op = operator(k, rate, padding, phase, v2)
        want_route = "bands" if name == "Gaussian_R1" and padding != "circular" else "kernel"
        assert op._op.route == want_route and op._op.separable == (name == "Gaussian_R1")
        y64, adj64, ct = reference64(image, k, padding, rate, phase, rule_of(padding, v2))
        g = ct.float().cuda()
        y, adj = op.A(image), transpose_to(op, g, (37, 50))
        assert y.shape == (2, 3, len(range(37)[phase::rate]), len(range(50)[phase::rate])) and adj.shape == image.shape
        # A_adjoint takes the image to be (rate h, rate w): float64 autograd on an image of those extents
        big = torch.zeros(2, 3, rate * y.shape[-2], rate * y.shape[-1])
        _, big64, _ = reference64(big, k, padding, rate, phase, rule_of(padding, v2), ct=ct)
        plain = op.A_adjoint(g)
        e_fwd, e_adj, e_plain = relerr(y, y64), relerr(adj, adj64), relerr(plain, big64)
        print(f"{name} {padding} v2={v2} rate {rate} phase {phase} ({want_route}): A {e_fwd:.2e} transpose at 37x50 "
              f"{e_adj:.2e} A_adjoint at {tuple(plain.shape[-2:])} {e_plain:.2e}")
        assert max(e_fwd, e_adj, e_plain) < TOL, (name, padding, v2, rate, phase, e_fwd, e_adj, e_plain)
        assert torch.equal(op.A_transpose(g), plain)


# ------------------------------------------------------------------ 2. the composition identities
@pytest.mark.parametrize("padding,v2", BOUNDARIES, ids=[f"{p}-{'v2' if v else 'legacy'}" for p, v in BOUNDARIES])
@pytest.mark.parametrize("name", ["rand5x4", "Gaussian_R1"])
def test_composition_identities(image, name, padding, v2):
    """A(x) is the blur's A(x)[..., o::s, o::s]; A_adjoint(g) the blur's A_adjoint of g zero-inserted at (o::s, o::s). Both
    sides are float32 sums of the same products in another order: the physics bar, relative to the blur's own result."""
    k = kernel_named(name)
    blur = blur_of(k, padding, v2)
    full = blur.A(image)
    for rate, phase in ((2, 0), (2, 1), (3, 2), (4, 0)):
        op = operator(k, rate, padding, phase, v2)
        y = op.A(image)
        g = torch.rand(y.shape, generator=torch.Generator().manual_seed(rate + phase)).cuda()
        up = torch.zeros_like(image)
        up[..., phase::rate, phase::rate] = g
        e_fwd = relerr(y, full[..., phase::rate, phase::rate])
        e_adj = relerr(transpose_to(op, g, (37, 50)), blur.A_adjoint(up))
        print(f"{name} {padding} v2={v2} rate {rate} phase {phase}: A {e_fwd:.2e} A_adjoint {e_adj:.2e}")
        assert e_fwd < TOL and e_adj < TOL, (name, padding, v2, rate, phase, e_fwd, e_adj)


@pytest.mark.parametrize("padding,v2", BOUNDARIES, ids=[f"{p}-{'v2' if v else 'legacy'}" for p, v in BOUNDARIES])
def test_rate_one_reproduces_the_blur(image, padding, v2):
    for name in ("rand5x4", "Gaussian_R1"):
        k = kernel_named(name)
        blur, op = blur_of(k, padding, v2), operator(k, 1, padding, 0, v2)
        y = op.A(image)
        assert y.shape == image.shape
        e_fwd, e_adj = relerr(y, blur.A(image)), relerr(op.A_adjoint(y), blur.A_adjoint(y))
        print(f"{name} {padding} v2={v2}: rate 1 against the blur: A {e_fwd:.2e} A_adjoint {e_adj:.2e}")
        assert e_fwd < TOL and e_adj < TOL


# ------------------------------------------------------------------ 3. tile, halo and wrap edges of the kernel
EDGES = [
    ("13x13 on 70x130 at rate 2: several tiles, partial last ones", (13, 13), (1, 2, 70, 130), 2, PADDINGS),
    ("63x3 at rate 4 on 40x72: the tallest footprint", (63, 3), (1, 1, 40, 72), 4, PADDINGS),
    ("5x5 on 5x6, n <= 2p", (5, 5), (1, 1, 5, 6), 2, ("replicate", "reflect")),
    ("circular 5x5 on 3x4: the kernel wraps more than once", (5, 5), (2, 1, 3, 4), 2, ("circular",)),
    ("63x63 at rate 8 on 64x256: the forward tile is halved to 1 x 16", (63, 63), (1, 1, 64, 256), 8, PADDINGS),
    ("4x6 on 33x47 at rate 3: even axes, n % s != 0", (4, 6), (2, 1, 33, 47), 3, PADDINGS),
]


@pytest.mark.parametrize("what,kshape,shape,rate,paddings", EDGES, ids=[e[0] for e in EDGES])
def test_kernel_edges_vs_float64(what, kshape, shape, rate, paddings):
    k = rand_kernel(*kshape, seed=sum(kshape))
    x = torch.rand(shape, generator=torch.Generator().manual_seed(2)).cuda()
    for padding in paddings:
        for phase in sorted({0, rate - 1}):
            op = operator(k, rate, padding, phase)
            assert op._op.route == "kernel"
            y64, adj64, ct = reference64(x, k, padding, rate, phase, rule_of(padding, True))
            e_fwd, e_adj = relerr(op.A(x), y64), relerr(transpose_to(op, ct.float().cuda(), shape[-2:]), adj64)
            print(f"{what}, {padding}, phase {phase}: A {e_fwd:.2e} A_adjoint {e_adj:.2e}")
            assert e_fwd < TOL and e_adj < TOL, (what, padding, phase, e_fwd, e_adj)


def test_extents_and_shapes_are_refused_by_name():
    x = torch.rand(1, 1, 5, 6, device="cuda")
    for k in (rand_kernel(13, 13, 1), torch.outer(rand_kernel(13, 1, 2)[:, 0], rand_kernel(1, 13, 3)[0])):
        with pytest.raises(ValueError, match="13 taps.*extent of 5 .*13x13"):
            operator(k, 2, "reflect").A(x)                            # p = 6 > n - 1
        assert operator(k, 2, "replicate").A(x).shape == (1, 1, 3, 3)
    op = operator(rand_kernel(5, 5, 4), 2, "replicate")
    y = op.A(torch.rand(1, 1, 9, 11, device="cuda"))
    assert y.shape == (1, 1, 5, 6)
    assert op.A_adjoint(y).shape == (1, 1, 10, 12)                    # without out_hw: (s h, s w)
    from physics._ops import apply_linear
    assert apply_linear(op._op, y, transpose=True, out_hw=(9, 11)).shape == (1, 1, 9, 11)
    with pytest.raises(ValueError, match="takes 4x6, got 5x6"):
        apply_linear(op._op, y, transpose=True, out_hw=(8, 11))


# ------------------------------------------------------------------ 4. the dot test
@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("kind", ["separable", "dense"])
def test_dot(kind, padding):
    import physics
    k = physics.get_kernel("Gaussian_R2") if kind == "separable" else rand_kernel(13, 13, 5)
    for rate, phase in ((2, 1), (4, 0)):
        op = operator(k, rate, padding, phase)
        gen = torch.Generator().manual_seed(8)
        x = torch.rand((2, 3, 70, 130), generator=gen).cuda()
        y = op.A(x)
        z = torch.rand(y.shape, generator=gen).cuda()
        lhs = (y.double() * z.double()).sum()
        rhs = (x.double() * transpose_to(op, z, (70, 130)).double()).sum()
        print(f"{kind} {padding} rate {rate}: <A x, g> {float(lhs):.10f} <x, A^T g> {float(rhs):.10f}")
        assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (kind, padding, rate, float(lhs), float(rhs))


# ------------------------------------------------------------------ 5. the same bits on every run
@pytest.mark.parametrize("padding", PADDINGS)
def test_adjoint_is_reproducible(padding):
    op = operator(rand_kernel(13, 13, 6), 2, padding)
    g = op.A(torch.rand(2, 3, 70, 130, device="cuda"))
    a = op.A_adjoint(g).clone()
    torch.cuda.synchronize()
    for _ in range(3):
        assert torch.equal(a, op.A_adjoint(g))


# ------------------------------------------------------------------ 6. autograd and capture
@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("kind", ["separable", "dense"])
def test_autograd_and_capture(kind, padding):
    import physics
    k = physics.get_kernel("Gaussian_R2") if kind == "separable" else rand_kernel(4, 6, 7)
    op = operator(k, 2, padding)
    gen = torch.Generator().manual_seed(9)
    x = torch.rand((2, 3, 40, 72), generator=gen).cuda().requires_grad_(True)
    y = op.A(x)
    assert y.shape == (2, 3, 20, 36)
    ct = torch.rand(y.shape, generator=gen).cuda().requires_grad_(True)
    (gx,) = torch.autograd.grad(y, x, ct, create_graph=True)
    assert torch.equal(gx, op.A_adjoint(ct))
    (gct,) = torch.autograd.grad(gx, ct, x.detach())                  # the backward of the adjoint is the operator
    assert torch.equal(gct, y)
    # after those eager calls the taps, bands and workspace exist: a capture holds launches only
    want_y, want_adj = y.detach().clone(), gx.detach().clone()
    sx, sct = x.detach().clone(), ct.detach().clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out_y, out_adj = op.A(sx), op.A_adjoint(sct)
    x2, ct2 = torch.rand_like(sx), torch.rand_like(sct)
    sx.copy_(x2)
    sct.copy_(ct2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_y, op.A(x2)) and torch.equal(out_adj, op.A_adjoint(ct2))
    assert torch.equal(op.A(x.detach()), want_y) and torch.equal(op.A_adjoint(ct.detach()), want_adj)


# ------------------------------------------------------------------ 7. inside the losses and the scripts
@pytest.mark.parametrize("method", ["proposed", "sure"])
def test_losses_match_a_float64_matrix_physics(method):
    """get_loss over the HIP BlurDownsampling (rate 2, Gaussian_R1, replicate) against the same loss classes over a test-local
    LinearPhysics whose A is M_v x M_h^T in float64 with the matrices of physics/_bands.blur_decimate_axis_matrix: loss to
    1e-4, weight-gradient norm to 1e-3."""
    import bench
    import models
    import physics
    from losses import get_loss
    from physics import _bands
    from physics._base import GaussianNoise, LinearPhysics

    args = bench.reference_args("cuda", hidden=8, scales=3, task="sr", sr_factor=2)
    args.method, args.blur_padding, args.sr_kernel, args.sr_phase = method, "replicate", "Gaussian_R1", 0
    p = physics.get_physics(args, "cuda")
    assert isinstance(p, physics.BlurDownsampling) and p.padding == "replicate" and p.rate == 2
    k = p.sr_filter.detach().cpu().double()[0, 0]
    tv, th = (k.sum(1) / k.sum()).numpy(), k.sum(0).numpy()
    mats = {}

    def axis(n, taps):
        if (n, id(taps)) not in mats:
            mats[n, id(taps)] = torch.from_numpy(_bands.blur_decimate_axis_matrix(n, taps, "replicate", 2, 0)).cuda()
        return mats[n, id(taps)]

    class MatrixPhysics(LinearPhysics):
        task = "sr"
        rate = 2

        def A(self, v):
            return (axis(v.shape[-2], tv) @ v.double() @ axis(v.shape[-1], th).T).float()

        def A_adjoint(self, v):
            return (axis(2 * v.shape[-2], tv).T @ v.double() @ axis(2 * v.shape[-1], th)).float()

    ref = MatrixPhysics()
    ref.noise_model = GaussianNoise(sigma=args.noise_level / 255)
    torch.manual_seed(0)
    model = models.get_model(args, p, "cuda").to("cuda").train()
    gen = torch.Generator().manual_seed(21)
    y = p(torch.rand((4, 3, 96, 96), generator=gen).cuda())
    assert y.shape == (4, 3, 48, 48)
    out = []
    draws = None
    for phys_ in (p, ref):
        lf = get_loss(args, phys_)
        if draws is None:
            torch.manual_seed(3)
            if method == "proposed":
                draws = lf.loss.draw(y, model)
                assert draws is not None and set(draws) == {"b", "rate", "center", "noise"}
            else:
                draws = {"b": torch.randn_like(y)}
        model.get_backbone().zero_grad_flat()
        val = lf.loss(x=None, y=y, model=model, draws=draws)
        val.backward()
        gn = torch.stack([q.grad.double().norm() for q in model.parameters()]).norm()
        out.append((float(val), float(gn)))
    (v1, g1), (v0, g0) = out
    print(f"{method}: loss {v1:.8f} vs {v0:.8f}, gradient norm {g1:.6e} vs {g0:.6e}")
    assert np.isfinite(v0) and g0 > 0
    assert abs(v1 - v0) / abs(v0) < 1e-4, (v1, v0)
    assert abs(g1 - g0) / g0 < 1e-3, (g1, g0)


def test_train_script_captures_the_step(tmp_path):
    out = tmp_path / "run"
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--device", "cuda", "--method", "proposed", "--task", "sr",
           "--sr_factor", "2", "--sr_kernel", "Gaussian_R1", "--blur_padding", "reflect", "--ProposedModel__architecture",
           "Convolutional", "--ConvolutionalModel__hidden_channels", "8", "--ConvolutionalModel__scales", "3", "--dataset",
           "synthetic", "--batch_size", "4", "--epochs", "4", "--max_steps", "2", "--checkpoint_interval", "2",
           "--out_dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, SEI_TRACE_STEP_KIND="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    rows = open(out / "training.csv").read().strip().splitlines()
    assert rows[0] == "Epoch,Training Loss" and len(rows) == 5
    assert all(np.isfinite(float(r_.split(",")[1])) for r_ in rows[1:])
    assert "step kind: hipGraph replay" in r.stdout, r.stdout


@pytest.mark.parametrize("kind", [["--model_kind", "Upsample"],
                                  ["--model_kind", "TV", "--tv_lambd", "0.01", "--tv_max_iter", "5"]], ids=["Upsample", "TV"])
def test_test_script_runs_the_baselines(kind):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), "--device", "cuda", "--task", "sr", "--sr_factor", "2",
                        "--sr_kernel", "Gaussian_R1", "--blur_padding", "reflect", "--dataset", "synthetic", "--indices",
                        "0,1"] + kind, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    psnr = float([ln for ln in r.stdout.splitlines() if ln.startswith("PSNR:")][0].split()[1])
    print(r.stdout.strip().splitlines()[-3:])
    assert np.isfinite(psnr), r.stdout
