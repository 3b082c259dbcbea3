"""physics.Blur with the replicate, reflect and valid boundaries on the GPU: every G19 case against the reference's own
outputs and against float64 F.pad + F.conv2d with its autograd, the tile and band edges of sei_blur_dense_pad, the dot
test, run-to-run bits, autograd and capture, and the operator inside the losses, train.py and test.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_blur_padding import G19_KERNELS, PADDINGS, SEPARABLE, g19

pytestmark = pytest.mark.gpu
TOL = 2e-6           # the physics bar of tests/test_physics_gpu.py: max-norm, relative to the float64 result's max-abs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def relerr(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def conv64(x, k, padding):
    """The reference's conv in float64 on the host: the filter flipped, zero-extended to an odd length (an even axis by
    one at its end, a single tap to three around it), the image padded by half of that with F.pad, then F.conv2d."""
    kv, kh = k.shape
    ev, eh = (3 if kv == 1 else kv + 1 - kv % 2), (3 if kh == 1 else kh + 1 - kh % 2)
    f = torch.zeros(ev, eh, dtype=torch.float64)
    ov, oh = int(kv == 1), int(kh == 1)
    f[ov:ov + kv, oh:oh + kh] = k.double().flip(0, 1)
    pv, ph = (ev - 1) // 2, (eh - 1) // 2
    if padding != "valid":
        x = F.pad(x, (ph, ph, pv, pv), mode=padding)
    b, c, h, w = x.shape
    return F.conv2d(x.reshape(b * c, 1, h, w), f[None, None]).reshape(b, c, h - 2 * pv, w - 2 * ph)


def reference64(x, k, padding, ct=None):
    """(A x, A^T ct) in float64: conv64 and its autograd (ct None: a random cotangent, returned third)."""
    x64 = x.detach().cpu().double().requires_grad_(True)
    y = conv64(x64, k.cpu(), padding)
    if ct is None:
        ct = torch.rand(y.shape, generator=torch.Generator().manual_seed(int(y.numel())))
    (gx,) = torch.autograd.grad(y, x64, ct.detach().cpu().double())
    return y.detach(), gx, ct


def blur(k, padding):
    import physics
    return physics.Blur(filter=k[None, None].cuda(), padding=padding, device="cuda")


def rand_kernel(kv, kh, seed):
    k = torch.rand((kv, kh), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return k / k.sum()


# ------------------------------------------------------------------ 1. the fixture
@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("name", G19_KERNELS)
def test_vs_reference_and_float64(golden, name, padding):
    g = g19(golden)
    k = torch.from_numpy(g[f"k.{name}"])
    op = blur(k, padding)
    if padding != "circular":
        assert op._op.separable == (name in SEPARABLE or min(k.shape) == 1)
    x, ct = dev(g["x"]), dev(g[f"{name}.{padding}.g"])
    y64, adj64, _ = reference64(x, k, padding, ct)
    y, adj = op.A(x), op.A_adjoint(ct)
    figures = {"A vs reference": relerr(y, g[f"{name}.{padding}.y"]), "A vs float64": relerr(y, y64),
               "A_adjoint vs reference": relerr(adj, g[f"{name}.{padding}.adj"]), "A_adjoint vs float64": relerr(adj, adj64)}
    own = max(relerr(g[f"{name}.{padding}.y"], y64), relerr(g[f"{name}.{padding}.adj"], adj64))
    print(f"{name} {padding}: " + ", ".join(f"{what} {e:.2e}" for what, e in figures.items())
          + f" (the reference's float32 against float64: {own:.2e})")
    assert all(e < TOL for e in figures.values()), (name, padding, figures)


# ------------------------------------------------------------------ 2. tile and band edges of the dense kernels
EDGES = [
    ("13x13 on 3 x 3 tiles, partial last tiles", (13, 13), (1, 2, 70, 130), ("replicate", "reflect", "valid")),
    ("63x3, p = 31: the far band straddles two tiles", (63, 3), (1, 1, 40, 72), ("replicate", "reflect")),        # (valid needs n > 2p)
    ("5x5 with n <= 2p", (5, 5), (1, 1, 5, 6), ("replicate", "reflect")),
    ("5x5 with n < p", (5, 5), (2, 1, 2, 9), ("replicate",)),
    ("valid with 4x6", (4, 6), (2, 3, 17, 21), ("valid",)),
]


@pytest.mark.parametrize("what,kshape,shape,paddings", EDGES, ids=[e[0] for e in EDGES])
def test_dense_kernel_edges_vs_float64(what, kshape, shape, paddings):
    k = rand_kernel(*kshape, seed=sum(kshape))
    x = torch.rand(shape, generator=torch.Generator().manual_seed(2)).cuda()
    for padding in paddings:
        op = blur(k, padding)
        assert not op._op.separable
        y64, adj64, ct = reference64(x, k, padding)
        e_fwd, e_adj = relerr(op.A(x), y64), relerr(op.A_adjoint(ct.cuda()), adj64)
        print(f"{what}, {padding}: A {e_fwd:.2e} A_adjoint {e_adj:.2e}")
        assert e_fwd < TOL and e_adj < TOL, (what, padding, e_fwd, e_adj)


def test_extents_the_boundary_cannot_take_are_refused_by_name():
    x = torch.rand(1, 1, 5, 6, device="cuda")
    for k in (rand_kernel(13, 13, 1), torch.outer(rand_kernel(13, 1, 2)[:, 0], rand_kernel(1, 13, 3)[0])):
        with pytest.raises(ValueError, match="extent of 5 .*13x13"):
            blur(k, "reflect").A(x)                                   # p = 6 > n - 1
        with pytest.raises(ValueError, match="valid.*13 taps"):
            blur(k, "valid").A(x)
        assert blur(k, "replicate").A(x).shape == x.shape
    # the adjoint of valid grows by 2p and says so when handed a gradient of another size
    op = blur(rand_kernel(5, 5, 4), "valid")
    y = op.A(torch.rand(1, 1, 9, 9, device="cuda"))
    assert y.shape == (1, 1, 5, 5) and op.A_adjoint(y).shape == (1, 1, 9, 9)


# ------------------------------------------------------------------ 3. the dot test
@pytest.mark.parametrize("padding", ["replicate", "reflect", "valid"])
@pytest.mark.parametrize("kind", ["separable", "dense"])
def test_dot(kind, padding):
    import physics
    k = physics.get_kernel("Gaussian_R2") if kind == "separable" else rand_kernel(13, 13, 5)
    op = blur(k, padding)
    assert op._op.separable == (kind == "separable")
    gen = torch.Generator().manual_seed(8)
    x = torch.rand((2, 3, 70, 130), generator=gen).cuda()
    y = op.A(x)
    z = torch.rand(y.shape, generator=gen).cuda()
    lhs, rhs = (y.double() * z.double()).sum(), (x.double() * op.A_adjoint(z).double()).sum()
    print(f"{kind} {padding}: <A x, g> {float(lhs):.10f} <x, A^T g> {float(rhs):.10f}")
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (kind, padding, float(lhs), float(rhs))


# ------------------------------------------------------------------ 4. the same bits on every run
@pytest.mark.parametrize("padding", ["replicate", "reflect", "valid"])
def test_dense_adjoint_is_reproducible(padding):
    op = blur(rand_kernel(13, 13, 6), padding)
    g = op.A(torch.rand(2, 3, 70, 130, device="cuda"))
    a = op.A_adjoint(g).clone()
    torch.cuda.synchronize()
    assert torch.equal(a, op.A_adjoint(g))


# ------------------------------------------------------------------ 5. autograd and capture
@pytest.mark.parametrize("padding", ["replicate", "reflect", "valid"])
@pytest.mark.parametrize("kind", ["separable", "dense"])
def test_autograd_and_capture(kind, padding):
    import physics
    k = physics.get_kernel("Gaussian_R2") if kind == "separable" else rand_kernel(4, 6, 7)
    op = blur(k, padding)
    gen = torch.Generator().manual_seed(9)
    x = torch.rand((2, 3, 40, 72), generator=gen).cuda().requires_grad_(True)
    y = op.A(x)
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


# ------------------------------------------------------------------ 6. inside the losses and the scripts
@pytest.mark.parametrize("method", ["proposed", "sure"])
def test_losses_match_a_float64_matrix_physics(method):
    """get_loss over the HIP Blur(padding='replicate') against the same loss classes over a test-local LinearPhysics whose A
    is M_v x M_h^T in float64 with the matrices of physics/_bands.blur_axis_matrix: loss to 1e-4, weight-gradient norm to
    1e-3 (the comparison and the bars of the loss-level test of tests/test_ct_like_filter_gpu.py)."""
    import bench
    import models
    import physics
    from losses import get_loss
    from physics import _bands
    from physics._base import GaussianNoise, LinearPhysics

    args = bench.reference_args("cuda", hidden=8, scales=3)
    args.method, args.blur_padding = method, "replicate"
    p = physics.get_physics(args, "cuda")
    assert isinstance(p, physics.Blur) and p.padding == "replicate"
    k = p.filter.detach().cpu().double()[0, 0]
    tv, th = (k.sum(1) / k.sum()).numpy(), k.sum(0).numpy()
    mats = {}

    def axis(n, taps):
        if (n, id(taps)) not in mats:
            mats[n, id(taps)] = torch.from_numpy(_bands.blur_axis_matrix(n, taps, "replicate")).cuda()
        return mats[n, id(taps)]

    class MatrixPhysics(LinearPhysics):
        task = "deblurring"
        filter = p.filter

        def A(self, v):
            return (axis(v.shape[-2], tv) @ v.double() @ axis(v.shape[-1], th).T).float()

        def A_adjoint(self, v):
            return (axis(v.shape[-2], tv).T @ v.double() @ axis(v.shape[-1], th)).float()

    ref = MatrixPhysics()
    ref.noise_model = GaussianNoise(sigma=args.noise_level / 255)
    torch.manual_seed(0)
    model = models.get_model(args, p, "cuda").to("cuda").train()
    gen = torch.Generator().manual_seed(21)
    y = p(torch.rand((4, 3, 48, 48), generator=gen).cuda())
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
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--device", "cuda", "--method", "proposed", "--task",
           "deblurring", "--kernel", "Gaussian_R2", "--blur_padding", "reflect", "--ProposedModel__architecture",
           "Convolutional", "--ConvolutionalModel__hidden_channels", "8", "--ConvolutionalModel__scales", "3", "--dataset",
           "synthetic", "--batch_size", "4", "--epochs", "4", "--max_steps", "2", "--checkpoint_interval", "2",
           "--out_dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, SEI_TRACE_STEP_KIND="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    rows = open(out / "training.csv").read().strip().splitlines()
    assert rows[0] == "Epoch,Training Loss" and len(rows) == 5
    assert all(np.isfinite(float(r_.split(",")[1])) for r_ in rows[1:])
    assert "step kind: hipGraph replay" in r.stdout, r.stdout


def test_test_script_runs_the_inverse_filter():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), "--device", "cuda", "--task", "deblurring",
                        "--kernel", "Gaussian_R1", "--blur_padding", "replicate", "--noise_level", "0", "--dataset",
                        "synthetic", "--indices", "0,1", "--model_kind", "InverseFilter"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    psnr = float([ln for ln in r.stdout.splitlines() if ln.startswith("PSNR:")][0].split()[1])
    print(r.stdout.strip().splitlines()[-3:])
    assert np.isfinite(psnr), r.stdout
