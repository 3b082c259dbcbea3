"""GPU: the TV-prox kernel (sei_tv_prox, through models.tv.tv_prox) and the TV baseline against the float64 restatement
of tests/test_tv_baseline.py; exactness of the kernel under splitting of its iterations and under every schedule;
determinism; test.py --model_kind TV end to end."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import physics
from models.tv import TV, tv_prox
from test_tv_baseline import (SIGMA, blur_circ, gaussian_r2, objective, piecewise_constant_case, psnr, tv_pgd_ref,
                              tv_prox_ref)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 1, 1, 1), (1, 1, 1, 7), (1, 2, 7, 1), (2, 3, 33, 47), (1, 3, 97, 131), (1, 1, 128, 64)]


def uniform(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("ths", [0.02, 0.5])
@pytest.mark.parametrize("shape", SHAPES)
def test_prox_kernel_matches_float64_restatement(shape, ths):
    """20 iterations from the cold start. x2 within 1e-5 max|ref| (the project's float32 operator bar); u2 within
    2 sigma 1e-5 = 2.5e-4 absolute (u is sigma times a difference of two x values)."""
    z = uniform(shape, seed=shape[-2] * 1000 + shape[-1])
    ref_x, (_, ref_u) = tv_prox_ref(z, ths, iters=20)
    x, (x2, u2) = tv_prox(z.float().cuda(), ths, iters=20)
    assert x.shape == z.shape and u2.shape == (2,) + tuple(z.shape) and torch.equal(x, x2)
    err_x = float((x.cpu().double() - ref_x).abs().max() / ref_x.abs().max())
    err_u = float((u2.cpu().double() - ref_u).abs().max())
    print(f"tv_prox {shape} ths {ths}: x2 rel {err_x:.2e}, u2 abs {err_u:.2e}")
    assert err_x < 1e-5
    assert err_u < 2 * SIGMA * 1e-5


@pytest.fixture(scope="module")
def split_case():
    z = uniform((1, 3, 97, 131), seed=5).float().cuda()
    x, (x2, u2) = tv_prox(z, 0.1, iters=20)
    return z, x2, u2


def advance(z, counts, **schedule):
    state = None
    for n in counts:
        _, state = tv_prox(z, 0.1, state, iters=n, **schedule)
    return state


@pytest.mark.parametrize("counts", [[1] * 20, [7, 13], [3, 5, 12]])
def test_iteration_splitting_is_exact(split_case, counts):
    """One call of 20 iterations (fused halo) against calls that split them, down to the one-ring path: the same bits."""
    z, x2, u2 = split_case
    got = advance(z, counts)
    assert torch.equal(got[0], x2) and torch.equal(got[1], u2)


@pytest.mark.parametrize("tile,k", [(64, 1), (64, 2), (64, 4), (64, 5), (64, 10), (64, 20), (32, 1), (32, 5), (32, 20)])
def test_every_schedule_gives_the_same_bits(split_case, tile, k):
    z, x2, u2 = split_case
    got = advance(z, [20], _tile=tile, _k=k)
    assert torch.equal(got[0], x2) and torch.equal(got[1], u2)
    got = advance(z, [7, 13], _tile=tile, _k=k)                # launches of fewer than k iterations stage a thinner halo
    assert torch.equal(got[0], x2) and torch.equal(got[1], u2)


def test_prox_is_deterministic_batch_independent_and_alignment_independent():
    z = uniform((2, 3, 97, 131), seed=9).float().cuda()
    a, (_, ua) = tv_prox(z, 0.1)
    b, (_, ub) = tv_prox(z, 0.1)
    assert torch.equal(a, b) and torch.equal(ua, ub)
    for i in range(2):
        one, (_, uo) = tv_prox(z[i], 0.1)
        assert torch.equal(one, a[i]) and torch.equal(uo, ua[:, i])
    buf = torch.zeros(1 + z.numel(), device="cuda")
    buf[1:] = z.flatten()
    zv = buf[1:].view(z.shape)                                  # contiguous, 4 bytes off the 16-byte grid
    assert zv.data_ptr() % 16 != 0
    c, (_, uc) = tv_prox(zv, 0.1)
    assert torch.equal(c, a) and torch.equal(uc, ua)
    d, _ = tv_prox(z.transpose(-1, -2).contiguous().transpose(-1, -2), 0.1)      # non-contiguous: staged
    assert torch.equal(d, a)
    with pytest.raises(TypeError):
        tv_prox(z.double(), 0.1)
    with pytest.raises(ValueError):
        tv_prox(z, 0.0)


def test_prox_continues_in_place_from_the_state_it_is_given():
    z = uniform((3, 33, 47), seed=3).float().cuda()
    _, state = tv_prox(z, 0.1, iters=7)
    x2_id, u2_id = state[0].data_ptr(), state[1].data_ptr()
    x, state = tv_prox(z, 0.1, state, iters=13)
    assert state[0].data_ptr() == x2_id and state[1].data_ptr() == u2_id and x.data_ptr() != x2_id
    ref, _ = tv_prox_ref(z.cpu().double(), 0.1, iters=20)
    assert float((x.cpu().double() - ref).abs().max() / ref.abs().max()) < 1e-5
    with pytest.raises(ValueError):
        tv_prox(z[:2], 0.1, state)


@pytest.fixture(scope="module")
def deblur_case():
    x, y = piecewise_constant_case()
    k = gaussian_r2()
    op = physics.BlurV2(kernel=physics.get_kernel("Gaussian_R2")[None, None].cuda())
    return x, y, k, op


@pytest.mark.parametrize("lambd", [0.02, 0.1])
def test_tv_deblurring_matches_float64_restatement(deblur_case, lambd):
    """30 outer iterations within 1e-4 max|ref| (the project's float32 end-to-end bar); the result lowers the objective
    and gains at least 1 dB over the measurement."""
    x, y, k, op = deblur_case
    A, At = (lambda v: blur_circ(v, k)), (lambda v: blur_circ(v, k, transpose=True))
    ref, ran, _ = tv_pgd_ref(y, A, At, lambd, max_iter=30, early_stop=False)
    model = TV(op, lambd=lambd, max_iter=30, early_stop=False)
    got = model(y.float().cuda()).cpu().double()
    err = float((got - ref).abs().max() / ref.abs().max())
    gain = psnr(got, x) - psnr(y, x)
    print(f"TV deblurring lambd {lambd}: rel {err:.2e}, gain {gain:.2f} dB")
    assert model.iterations_run == ran == 30 and got.shape == x.shape
    assert err < 1e-4
    assert objective(got, y, A, lambd) < objective(At(y), y, A, lambd)
    assert gain >= 1.0


def test_tv_super_resolution_matches_float64_restatement():
    from physics import _bands
    op = physics.Downsampling(rate=2, antialias=True)
    g = torch.Generator().manual_seed(4)
    y = torch.rand((1, 3, 20, 28), generator=g, dtype=torch.float64)
    dv, dh = (torch.from_numpy(np.asarray(_bands.aa_bicubic_matrix(n, 1 / 2), dtype=np.float64)) for n in (40, 56))
    uv, uh = (torch.from_numpy(np.asarray(_bands.plain_bicubic_matrix(n, 2), dtype=np.float64)) for n in (20, 28))
    A = lambda v: dv @ v @ dh.T                                  # noqa: E731
    At = lambda v: uv @ v @ uh.T                                 # noqa: E731  (the reference's deprecated adjoint)
    ref, _, _ = tv_pgd_ref(y, A, At, 0.02, max_iter=30, early_stop=False)
    model = TV(op, lambd=0.02, max_iter=30, early_stop=False)
    got = model(y.float().cuda()).cpu().double()
    assert got.shape == (1, 3, 40, 56)
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"TV sr x2: rel {err:.2e}")
    assert err < 1e-4


def test_early_stop(deblur_case):
    x, y, k, op = deblur_case
    model = TV(op, lambd=0.02)
    flat = model(torch.full((1, 3, 40, 56), 0.5, device="cuda"))
    assert model.iterations_run == 3
    assert float((flat - 0.5).abs().max()) < 1e-6
    model = TV(op, lambd=0.02, max_iter=12)
    model(y.float().cuda())
    assert model.iterations_run == 12


COMMON = ["--device", "cuda", "--dataset", "synthetic", "--indices", "0,1", "--model_kind", "TV"]


def run_test_py(*flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), *COMMON, *flags], capture_output=True, text=True,
                          timeout=300)


@pytest.mark.parametrize("task", [["--task", "deblurring", "--kernel", "Gaussian_R2"], ["--task", "sr", "--sr_factor", "2"]])
def test_test_py_runs_the_tv_baseline(task):
    r = run_test_py(*task, "--tv_lambd", "0.02", "--tv_max_iter", "20")
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert "N: 2" in lines
    assert math.isfinite(float([ln for ln in lines if ln.startswith("PSNR:")][0].split()[-1]))


def test_test_py_names_the_missing_flag():
    r = run_test_py("--task", "deblurring", "--kernel", "Gaussian_R2")
    assert r.returncode != 0 and "--tv_lambd" in r.stderr
