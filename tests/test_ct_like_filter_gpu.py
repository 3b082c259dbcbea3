"""CTLikeFilter on the GPU (sei_circ_filter_sep): against the reference's own outputs (G16), against the float64 dense
circulants at shapes the fixture does not hold, as an operator (symmetry, exact inverse), through get_physics, inside the
losses, and through train.py / test.py with --task invert_a_tomography_like_filter."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_ct_like_filter import TAGS, g16

pytestmark = pytest.mark.gpu
TOL = 2e-6           # the physics bar of tests/test_physics_gpu.py: max-norm, relative to the reference's max-abs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASK = "invert_a_tomography_like_filter"


def relerr(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def circ(n, inverse, dtype=torch.float64):
    from physics import _circulant
    return torch.from_numpy(_circulant.dense(n, inverse)).to("cuda", dtype)


def dense_apply(x, inverse, dtype=torch.float64):
    """C_H x C_W^T by torch.matmul on the GPU in `dtype` (the matrices rounded from float64)."""
    return circ(x.shape[-2], inverse, dtype) @ x.to(dtype) @ circ(x.shape[-1], inverse, dtype).T


@pytest.fixture(scope="module")
def op():
    import physics
    return physics.CTLikeFilter()


@pytest.mark.parametrize("tag", list(TAGS))
def test_vs_golden(golden, op, tag):
    g = g16(golden)
    ref32 = relerr(g[f"{tag}.f32.A"], g[f"{tag}.f64.A"])          # the reference's own float32 (FFT) error
    x = dev(g[f"{tag}.f32.x"]).requires_grad_(True)
    y, yd = op.A(x), op.A_dagger(x)
    e_a, e_d = relerr(y, g[f"{tag}.f64.A"]), relerr(yd, g[f"{tag}.f64.Adag"])
    print(f"{tag}: A {e_a:.2e} A_dagger {e_d:.2e} (reference in float32: A {ref32:.2e})")
    assert e_a < TOL and e_d < TOL, (tag, e_a, e_d, "reference float32", ref32)
    if tag == "big":
        return
    ct = dev(g[f"{tag}.f32.ct"])
    (gx,) = torch.autograd.grad(y, x, ct)
    (gxd,) = torch.autograd.grad(yd, x, ct)
    e_g, e_gd = relerr(gx, g[f"{tag}.f64.gA"]), relerr(gxd, g[f"{tag}.f64.gAdag"])
    e_adj = relerr(op.A_adjoint(ct), g[f"{tag}.f64.gA"])
    print(f"{tag}: vjp A {e_g:.2e} vjp A_dagger {e_gd:.2e} A_adjoint {e_adj:.2e}")
    assert e_g < TOL and e_gd < TOL and e_adj < TOL, (tag, e_g, e_gd, e_adj, "reference float32", ref32)
    if tag in ("rect", "odd"):
        e2 = relerr(op.filter1d(x.detach(), dim=2, inverse=True), g[f"{tag}.f64.f1d_dim2_inv"])
        e3 = relerr(op.filter1d(x.detach(), dim=3, inverse=False), g[f"{tag}.f64.f1d_dim3_fwd"])
        print(f"{tag}: filter1d dim 2 {e2:.2e} dim 3 {e3:.2e}")
        assert e2 < TOL and e3 < TOL, (tag, e2, e3)
        assert torch.equal(op.filter1d(x.detach(), dim=-1, inverse=False), op.filter1d(x.detach(), dim=3, inverse=False))
        with pytest.raises(ValueError):
            op.filter1d(x.detach(), dim=1)


@pytest.mark.parametrize("shape", [(8, 3, 256, 256), (1, 3, 256, 385), (3, 3, 65, 130), (32, 3, 48, 48), (1, 1, 512, 512)])
def test_vs_dense_circulants(op, shape):
    """Extents <= 385: the 2e-6 bar. 512 x 512 (the largest extent the entry point is required to run, 137 KiB of LDS):
    no fixed bar; at most twice the error of the same product by float32 torch.matmul on the same GPU."""
    gen = torch.Generator().manual_seed(16)
    x = torch.rand(shape, generator=gen).cuda()
    for inverse, fn in ((True, op.A), (False, op.A_dagger)):
        ref = dense_apply(x, inverse)
        err = relerr(fn(x), ref)
        if max(shape[-2:]) <= 385:
            print(f"{shape} inverse={inverse}: {err:.2e}")
            assert err < TOL, (shape, inverse, err)
        else:
            mm = relerr(dense_apply(x, inverse, torch.float32), ref)
            print(f"{shape} inverse={inverse}: kernel {err:.2e}, float32 torch.matmul {mm:.2e}")
            assert err <= 2 * mm, (shape, inverse, err, mm)


def test_beyond_the_lds_budget_is_refused(op):
    import _native
    with pytest.raises(_native.NativeLibraryError, match="SEI_ERR_TOO_LARGE"):
        op.A(torch.zeros(1, 1, 8, 2048, device="cuda"))


def matmul_round_trip(x):
    """A_dagger(A(x)) with both operators as float32 torch.matmul on the GPU, against x."""
    return relerr(dense_apply(dense_apply(x, True, torch.float32), False, torch.float32), x)


def test_symmetry_and_exact_inverse(op):
    """<A x, z> = <x, A z>, and the two round trips at 256 x 256. A(A_dagger(x)) = x to 1e-4. A_dagger(A(x)) = x cannot
    meet 1e-4 in float32 whatever computes it: the ramp's gain is up to (n/2 + 1)^2 = 16641, and rounding the exact A(x)
    to float32 alone, with A_dagger exact, already leaves 3.4e-4 (numpy, float64 around one float32 rounding; float32
    matmul on the CPU: 3.1e-3 for A_dagger(A(x)), 1.5e-5 for A(A_dagger(x))). Its bar is therefore 4x the round trip of
    float32 torch.matmul on the same GPU. The test prints all three figures before it asserts. Measured on an MI355X:
    A_dagger(A(x)) 1.86e-3 (so 1e-4 does not hold) with the torch.matmul round trip at 3.27e-3, A(A_dagger(x)) 1.54e-5."""
    gen = torch.Generator().manual_seed(17)
    x, z = (torch.rand((2, 3, 256, 256), generator=gen).cuda() for _ in range(2))
    for fn in (op.A, op.A_dagger, op.A_adjoint):
        lhs, rhs = (fn(x).double() * z.double()).sum(), (x.double() * fn(z).double()).sum()
        assert abs(lhs - rhs) / abs(lhs) < 1e-6, (fn.__name__, float(lhs), float(rhs))
    e1, e2 = relerr(op.A_dagger(op.A(x)), x), relerr(op.A(op.A_dagger(x)), x)
    mm = matmul_round_trip(x)
    print(f"round trips: A_dagger(A(x)) {e1:.2e}, A(A_dagger(x)) {e2:.2e}; float32 torch.matmul A_dagger(A(x)) {mm:.2e}; "
          f"gain bound {(256 / 2 + 1) ** 2:.0f}")
    assert e2 < 1e-4, (e2, mm)
    assert e1 <= 4 * mm, (e1, mm)


def _physics_args(noise_level=5):
    return argparse.Namespace(task=TASK, kernel=None, sr_factor=None, noise_level=noise_level, physics_v2=True,
                              physics_true_adjoint=False)


def test_physics_manager_surface():
    import physics
    p = physics.get_physics(_physics_args(), device="cuda")
    assert isinstance(p, physics.CTLikeFilter) and p.task == TASK
    assert not hasattr(p, "rate") and not hasattr(p, "filter")
    assert abs(p.noise_model.sigma - 5 / 255) < 1e-12
    mgr = getattr(p, "__manager")
    assert mgr.task == TASK and mgr.get_physics() is p
    x = torch.rand(1, 3, 32, 40, device="cuda")
    torch.manual_seed(123)
    before = torch.cuda.get_rng_state()
    a = mgr.randomly_degrade(x, seed=7)
    b = mgr.randomly_degrade(x, seed=7)
    assert torch.equal(a, b)                                       # deterministic per seed
    assert torch.equal(torch.cuda.get_rng_state(), before)         # and the global stream is untouched
    resid = (a - p.A(x)).std().item()
    assert 0.5 * 5 / 255 < resid < 1.5 * 5 / 255
    assert p(x).shape == x.shape


def test_inverse_filter_model_kind_is_the_exact_inverse():
    import bench
    import models
    import physics
    args = bench.reference_args("cuda", hidden=8, scales=3, task=TASK)
    args.model_kind = "InverseFilter"
    p = physics.get_physics(args, "cuda")
    model = models.get_model(args, p, "cuda")
    x = torch.rand(2, 3, 48, 64, device="cuda")
    err, mm = relerr(model(p.A(x)), x), matmul_round_trip(x)
    print(f"InverseFilter(A(x)) vs x: {err:.2e}; float32 torch.matmul round trip {mm:.2e}")
    assert err <= 4 * mm, (err, mm)                # the bar of test_symmetry_and_exact_inverse for this direction


@pytest.mark.parametrize("method", ["proposed", "sure"])
def test_losses_match_a_float64_matmul_physics(method):
    """get_loss over the HIP CTLikeFilter against the same loss classes over a test-local LinearPhysics whose A is the
    float64 dense product in torch: loss to 1e-4, weight-gradient norm to 1e-3 (the bars of the G15 test)."""
    import bench
    import models
    import physics
    from losses import get_loss
    from physics._base import GaussianNoise, LinearPhysics

    class DensePhysics(LinearPhysics):
        task = TASK

        def A(self, v):
            return dense_apply(v, True).float()

        A_adjoint = A

    args = bench.reference_args("cuda", hidden=8, scales=3, task=TASK)
    args.kernel, args.method, args.sure_margin = None, method, 0
    p = physics.get_physics(args, "cuda")
    ref = DensePhysics()
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
                assert lf.loss.sure.margin == 0
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


@pytest.mark.parametrize("n", [48, 256])
def test_the_tap_cache_is_warm_after_one_call_and_capturable(n):
    """The first call at an extent uploads the first columns (and, above 64 KiB of LDS -- 256 x 256 -- raises the kernel's
    LDS allowance); later calls launch only: a step captured after an eager warm-up call holds the kernel and nothing else."""
    import physics
    from physics import _ops
    op = physics.CTLikeFilter()
    x = torch.rand(2, 3, n, n, device="cuda")
    want = op.A(x)
    keys = set(_ops._CIRCULANT_COLUMNS)
    assert (n, True, 1.0, x.device) in keys                        # one column serves H and W of a square image
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    static = x.clone()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = op.A(static)
    assert set(_ops._CIRCULANT_COLUMNS) == keys
    x2 = torch.rand(2, 3, n, n, device="cuda")
    static.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, op.A(x2)) and torch.equal(op.A(x), want)


def test_train_script_captures_the_step(tmp_path):
    out = tmp_path / "run"
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--device", "cuda", "--method", "proposed", "--task", TASK,
           "--sure_margin", "0", "--ProposedModel__architecture", "Convolutional",
           "--ConvolutionalModel__hidden_channels", "8", "--ConvolutionalModel__scales", "3", "--dataset",
           "synthetic", "--batch_size", "4", "--epochs", "4", "--max_steps", "2", "--checkpoint_interval", "2",
           "--out_dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, SEI_TRACE_STEP_KIND="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    rows = open(out / "training.csv").read().strip().splitlines()
    assert rows[0] == "Epoch,Training Loss" and len(rows) == 5
    assert all(np.isfinite(float(r_.split(",")[1])) for r_ in rows[1:])
    assert "step kind: hipGraph replay" in r.stdout, r.stdout
    # the default margin does not exist for this task: the driver says which flags decide it
    r = subprocess.run([c for c in cmd if c not in ("--sure_margin", "0")], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--sure_margin N" in r.stderr, r.stdout + r.stderr


def test_test_script_inverse_filter_beats_identity():
    psnr = {}
    for kind in ("InverseFilter", "Identity"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), "--device", "cuda", "--task", TASK,
                            "--noise_level", "0", "--dataset", "synthetic", "--indices", "0,1", "--model_kind", kind],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        psnr[kind] = float([ln for ln in r.stdout.splitlines() if ln.startswith("PSNR:")][0].split()[1])
        assert np.isfinite(psnr[kind]), r.stdout
    print(psnr)
    assert psnr["InverseFilter"] > psnr["Identity"], psnr
