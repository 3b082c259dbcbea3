"""GPU: the sei_cg_* conjugate-gradient kernels against a float64 CG and for their stopping behaviour, sei_diffpir_sample
and the DiffPIR prologue of sei_cg_init against the literal float64 expressions, the DiffPIR model of models/diffpir.py in both
arithmetic modes and on both conjugate-gradient paths against the float64 restatement of tests/diffpir_ref.py, and
test.py --model_kind DiffPIR_DRUNet end to end."""
import math
import os
import subprocess
import sys

import pytest
import torch

import _native as N
import physics
from diffpir_ref import cg_history_ref, diffpir_ref, prologue_ref, sample_ref, tables_ref
from drunet_ref import cg_ref, synthetic_state_dict
from models._cg import FusedCG
from models.diffpir import DiffPIR
from models.drunet import DRUNet
from test_pnp_baseline_gpu import _pnp_case
from test_tv_baseline import blur_circ, gaussian_r2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24                         # float32 unit roundoff
# n -> an image shape with that many elements: below one 16-byte lane, below one workgroup, odd tails (105 = 26 quads + 1,
# 4653 = 1163 quads + 1: five workgroups; 73731 = 72 full workgroups + 3), whole quads (6720: seven workgroups)
SHAPES = {1: (1, 1, 1, 1), 3: (1, 1, 1, 3), 105: (1, 3, 5, 7), 4653: (1, 3, 33, 47), 6720: (1, 3, 40, 56),
          73731: (1, 3, 7, 3511)}
SIZES = sorted(SHAPES)


def rand64(shape, seed, normal=False):
    """float64 values that float32 holds exactly."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) if normal else torch.rand(shape, generator=g)).double()


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))       # (NaN-proof)


def state_of(cg):
    words = cg.state.cpu()
    rs, pAp, rs_new = words[:3].view(torch.float32).tolist()
    return dict(rs=rs, pAp=pAp, rs_new=rs_new, done=int(words[N.CG_DONE]), iterations=int(words[N.CG_ITERATIONS]))


# ---- conjugate gradients ----

@pytest.fixture(scope="module")
def blur():
    return physics.BlurV2(kernel=physics.get_kernel("Gaussian_R2")[None, None].cuda())


def _cg_inputs(n, seed):
    return rand64(SHAPES[n], seed), rand64(SHAPES[n], seed + 1000)


def _cg_errors(n, seed, iters, gamma, k):
    """(float64 solution, relative max-norm error of the float32 CPU run) of `iters` CG iterations on blur^T blur + I / gamma."""
    u0, Aty = _cg_inputs(n, seed)
    out = []
    for dt in (torch.float64, torch.float32):
        kk = k.to(dt)
        op = lambda v: blur_circ(blur_circ(v, kk), kk, transpose=True) + v / gamma      # noqa: E731
        out.append(cg_ref(op, Aty.to(dt) + u0.to(dt) / gamma, iters, 0.0).double())
    return out[0], float((out[1] - out[0]).abs().max() / out[0].abs().max())


@pytest.mark.parametrize("n", SIZES)
def test_cg_matches_float64(blur, n):
    """tol = 0 and 12 iterations on blur^T blur + I / gamma (Gaussian_R2, circular), gamma = 2 (a power of two: u0 / gamma
    and u0 * (1 / gamma) are the same float): the error of x against the float64 CG is at most 4x that of the same CG in
    float32 on the CPU, and a second run gives the same bits.

    n = 1 and n = 3: on 1 x 1 the operator has one eigenvalue and on 1 x 3 two (the blur is symmetric), so CG is exact after
    1 and 2 iterations; run on, deepinv's recurrences reach r = 0 and then 0 / 0 in every arithmetic, the float64 one
    included, and there is nothing left to compare. For these two sizes the comparison is made after 1 and 2 iterations,
    and the 12-iteration run is still made and held to bit-identity. With one to three unknowns the error of a single
    float32 run is a handful of roundings, 0 to 2 ulps by chance, so the float32 CPU error is taken as the worst over 64
    draws of the inputs there, and the GPU is held to it on each of the first 8."""
    gamma, k = 2.0, gaussian_r2()
    iters = {1: 1, 3: 2}.get(n, 12)
    draws = 64 if n < 105 else 1
    refs = [_cg_errors(n, seed, iters, gamma, k) for seed in range(draws)]
    e_cpu = max(e for _, e in refs)
    shape = SHAPES[n]
    op = lambda p, out: blur.A_adjoint(blur.A(p.view(shape)).contiguous()).contiguous()      # noqa: E731
    cg = FusedCG(n, torch.device("cuda", 0))
    for seed in range(min(draws, 8)):
        u0, Aty = (t.float().cuda() for t in _cg_inputs(n, seed))
        x = cg.solve(op, u0, Aty, gamma, iters, 0.0).clone()
        assert cg.iterations == iters == cg.launched and x.shape == (n,)
        ref = refs[seed][0]
        e_gpu = float((x.cpu().double().view(shape) - ref).abs().max() / ref.abs().max())
        print(f"CG n={n} seed {seed}: {iters} iterations, error {e_gpu:.3e} (float32 cpu {e_cpu:.3e})")
        assert e_gpu <= 4 * e_cpu
        again = cg.solve(op, u0, Aty, gamma, iters, 0.0)
        assert same_bits(x, again)
        # another solver object, other buffers: the same bits
        assert same_bits(x, FusedCG(n, torch.device("cuda", 0)).solve(op, u0, Aty, gamma, iters, 0.0))
    u0, Aty = (t.float().cuda() for t in _cg_inputs(n, 0))
    long = cg.solve(op, u0, Aty, gamma, 12, 0.0).clone()
    assert cg.iterations == 12 and same_bits(long, cg.solve(op, u0, Aty, gamma, 12, 0.0))


def _stopping_case(n):
    """Diagonal A^T A with the eigenvalues 0.5, 1, 2 in turn, gamma = 1 (the solve's operator has 1.5, 2, 3), and a right-hand
    side of norm 10 split into Aty + u0."""
    d = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64).repeat((n + 2) // 3)[:n]
    u0, Aty = rand64((n,), 11), rand64((n,), 12)
    s = 10.0 / float(torch.linalg.vector_norm(u0 + Aty))
    return d, (u0 * s).float().double(), (Aty * s).float().double()


@pytest.mark.parametrize("n", [3, 105, 4653, 73731])
def test_cg_stops_on_the_device(n):
    """Three distinct eigenvalues: CG converges in three iterations. The residual norm is far above tol after the second
    and far below it after the third, in float64 and in float32, so the count is not marginal; the device then counts 3,
    x is bit for bit the x of three iterations without a stopping test, and `poll` changes nothing."""
    tol = 1e-3
    d, u0, Aty = _stopping_case(n)
    for dt in (torch.float64, torch.float32):
        dd = d.to(dt)
        _, norms = cg_history_ref(lambda v: dd * v + v, Aty.to(dt) + u0.to(dt), 3)
        print(f"stopping n={n} {dt}: residual norms {norms}")
        assert norms[1] > 10 * tol and norms[2] < tol / 10
    dev = torch.device("cuda", 0)
    dg, u0g, Atyg = d.float().cuda(), u0.float().cuda(), Aty.float().cuda()

    def op(p, out):
        return torch.mul(dg, p, out=out)

    cg = FusedCG(n, dev)
    three = cg.solve(op, u0g, Atyg, 1.0, 3, 0.0).clone()
    assert cg.iterations == 3 and state_of(cg)["done"] == 0
    for poll, launched in ((1, 3), (5, 5), (50, 50)):
        x = cg.solve(op, u0g, Atyg, 1.0, 50, tol, poll=poll)
        st = state_of(cg)
        assert cg.iterations == 3 == st["iterations"] and st["done"] == 1 and cg.launched == launched
        assert math.sqrt(st["rs_new"]) < tol
        assert same_bits(x, three), poll
    # the solution itself: (d + 1) x = b
    want = (Aty + u0) / (d + 1)
    assert float((three.cpu().double() - want).abs().max() / want.abs().max()) < 1e-5


# ---- the sampling kernel and the prologue ----

def _schedule_scalars(t, tn):
    sa, s1m, _, srec = tables_ref()
    return dict(sa_t=float(sa[t]), s1m_t=float(s1m[t]), sa_n=float(sa[tn]), s1m_n=float(s1m[tn]), zeta=0.1,
                at_n=1.0 / float(srec[tn]) ** 2)


def _sample_inputs(n, seed):
    return rand64((n,), seed), rand64((n,), seed + 1, normal=True), rand64((n,), seed + 2, normal=True)


STEPS = [(999, 422), (183, 0)]           # the first and the last sampling step of a four-step schedule


@pytest.fixture(scope="module")
def sample_factor():
    """{step: (F_x, F_in)}: the float32 CPU evaluation's worst error against float64 over 73731 elements, in units of
    2^-24 times the element's largest operand."""
    out = {}
    for step in STEPS:
        c = _schedule_scalars(*step)
        u, x, nz = _sample_inputs(73731, 5)
        xn, xin, big, big_in = sample_ref(u, x, nz, **c)
        xn32, xin32, _, _ = sample_ref(u.float(), x.float(), nz.float(), **c)
        out[step] = (float(((xn32.double() - xn).abs() / (U32 * big)).max()),
                     float(((xin32.double() - xin).abs() / (U32 * big_in)).max()))
    return out


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("n", SIZES)
def test_sample_kernel(sample_factor, n, step):
    """|error| <= 4 F 2^-24 (largest operand of the element), F measured on the float32 CPU evaluation of the same
    expressions (a few: the chain is a dozen operations)."""
    c = _schedule_scalars(*step)
    fx, fin = sample_factor[step]
    assert 0.5 <= fx <= 16 and 0.5 <= fin <= 16, (fx, fin)
    u, x, nz = _sample_inputs(n, 40 + n)
    xn, xin, big, big_in = sample_ref(u, x, nz, **c)
    ug, xg, zg = u.float().cuda(), x.float().cuda(), nz.float().cuda()
    og = torch.full((n,), 7.0, device="cuda")
    N.call("sei_diffpir_sample", ug.data_ptr(), xg.data_ptr(), zg.data_ptr(), og.data_ptr(), c["sa_t"], c["s1m_t"],
           c["sa_n"], c["s1m_n"], c["zeta"], c["at_n"], n)
    ex = float(((xg.cpu().double() - xn).abs() / (U32 * big)).max())
    ei = float(((og.cpu().double() - xin).abs() / (U32 * big_in)).max())
    print(f"sample n={n} step {step}: x {ex:.2f} (float32 cpu {fx:.2f}), input {ei:.2f} (float32 cpu {fin:.2f}) "
          "x 2^-24 x largest operand")
    assert ex <= 4 * fx and ei <= 4 * fin
    assert torch.equal(ug.cpu().double(), u) and torch.equal(zg.cpu().double(), nz)        # read only


def _prologue_inputs(n, seed):
    """Denoiser outputs in (-0.5, 1.5), the first entries pinned below 0, above 1 and inside: both clamp branches and the
    pass-through are reached at every n >= 3 (n = 1 takes the three one by one)."""
    pins = torch.tensor([-0.3, 1.4, 0.6], dtype=torch.float64).float().double()
    if n == 1:
        return [pins[i:i + 1] for i in range(3)]
    o = rand64((n,), seed) * 2 - 0.5
    o[:3] = pins
    return [o]


@pytest.fixture(scope="module")
def prologue_factor():
    inv_gamma = float(torch.tensor(53.8).float())
    o, a = _prologue_inputs(73731, 5)[0], rand64((73731,), 6)
    b, b32 = prologue_ref(o, a, inv_gamma), prologue_ref(o.float(), a.float(), inv_gamma).double()
    return inv_gamma, float(((b32 - b).abs() / (U32 * _prologue_operands(o, a, b, inv_gamma))).max())


def _prologue_operands(o, a, b, inv_gamma):
    u = (2 * o - 1).clamp(-1, 1) / 2 + 0.5
    return torch.stack([(2 * o).abs(), (2 * o - 1).abs(), u.abs(), (u * inv_gamma).abs(), a.abs(), b.abs()]).amax(0)


@pytest.mark.parametrize("n", SIZES)
def test_cg_init_with_the_diffpir_prologue(prologue_factor, n):
    inv_gamma, f = prologue_factor
    assert 0.5 <= f <= 16, f
    below = above = inside = False
    for o in _prologue_inputs(n, 60 + n):
        a = rand64((n,), 61 + n)
        v = 2 * o - 1
        below, above, inside = below or bool((v < -1).any()), above or bool((v > 1).any()), inside or bool((v.abs() < 1).any())
        b = prologue_ref(o, a, inv_gamma)
        cg = FusedCG(n, torch.device("cuda", 0))
        for t in (cg.x, cg.r, cg.p):
            t.fill_(9.0)
        og, ag = o.float().cuda(), a.float().cuda()
        N.call("sei_cg_init", og.data_ptr(), ag.data_ptr(), inv_gamma, 1, cg.x.data_ptr(),
               cg.r.data_ptr(), cg.p.data_ptr(), cg.part.data_ptr(), cg.state.data_ptr(), n)
        err = float(((cg.p.cpu().double() - b).abs() / (U32 * _prologue_operands(o, a, b, inv_gamma))).max())
        print(f"prologue n={n}: {err:.2f} (float32 cpu {f:.2f}) x 2^-24 x largest operand")
        assert err <= 4 * f
        assert same_bits(cg.r, cg.p) and float(cg.x.abs().max()) == 0.0
        st = state_of(cg)
        rs64 = float((cg.p.cpu().double() ** 2).sum())
        assert abs(st["rs"] - rs64) <= (n + 2) * U32 * rs64 and st["done"] == 0 and st["iterations"] == 0
        # without the prologue u0 is taken as it is
        N.call("sei_cg_init", og.data_ptr(), ag.data_ptr(), inv_gamma, 0, cg.x.data_ptr(),
               cg.r.data_ptr(), cg.p.data_ptr(), cg.part.data_ptr(), cg.state.data_ptr(), n)
        plain = (a.float() + o.float() * torch.tensor(inv_gamma).float()).cuda()
        assert same_bits(cg.p, plain)
        assert torch.equal(og.cpu().double(), o) and torch.equal(ag.cpu().double(), a)      # read only
    assert below and above and inside


# ---- the model ----

@pytest.fixture(scope="module")
def net():
    sd = synthetic_state_dict(nb=1, seed=1)
    model = DRUNet(nb=1)
    model.load_state_dict(sd)
    return sd, model.cuda().eval()


class Noise:
    sigma = 5 / 255


@pytest.mark.parametrize("kind", ["deblurring", "sr"])
def test_diffpir_matches_float64_restatement(net, kind):
    """nb = 1, max_iter = 6, cg_tol = 0 and cg_max_iter = 12 so that both sides run the same iteration counts, the same noise
    tensors on both sides, sigma = 5 / 255. f32 mode: the error against float64 is at most 4x that of the float32 CPU
    chain, and the fused and the literal conjugate-gradient paths agree within that bound. The default bf16 mode stays
    within 4x the distance that rounding to bf16 moves the float32 CPU chain, and is finite."""
    sd, drunet = net
    y, op, A, At = _pnp_case(kind)
    op.noise_model = Noise()
    x_shape = tuple(At(torch.float64)(y).shape)
    draws = {i: rand64(x_shape, 100 + i, normal=True) for i in range(7)}
    kw = dict(max_iter=6, cg_max_iter=12, cg_tol=0.0)
    ref, proxes = diffpir_ref(y, A(torch.float64), At(torch.float64), sd, Noise.sigma, torch.float64, draws, **kw)
    cpu32, _ = diffpir_ref(y, A(torch.float32), At(torch.float32), sd, Noise.sigma, torch.float32, draws, **kw)
    cpu16, _ = diffpir_ref(y, A(torch.float32), At(torch.float32), sd, Noise.sigma, torch.float32, draws, round_bf16=True, **kw)
    scale = float(ref.abs().max())
    assert proxes == 5 and 0.0 <= float(ref.min()) and float(ref.max()) <= 1.0

    class Fixed(DiffPIR):
        def draw(self, i, like):
            return draws[i].float().to(like.device)

    out = {}
    for mode, fused in (("f32", True), ("bf16", True), ("f32", False)):
        model = Fixed(op, drunet, fused_cg=fused, **kw)
        assert len(model.state_dict()) == 0
        drunet.compute_dtype = mode
        out[mode, fused] = model(y.float().cuda()).cpu().double()
        assert out[mode, fused].shape == ref.shape
        assert model.cg_iterations == [12] * 5
    drunet.compute_dtype = "bf16"
    e_gpu = float((out["f32", True] - ref).abs().max()) / scale
    e_lit = float((out["f32", False] - ref).abs().max()) / scale
    e_cpu = float((cpu32.double() - ref).abs().max()) / scale
    d_paths = float((out["f32", True] - out["f32", False]).abs().max()) / scale
    d_gpu = float((out["bf16", True] - out["f32", True]).abs().max()) / scale
    d_cpu = float((cpu16.double() - cpu32.double()).abs().max()) / scale
    print(f"DiffPIR {kind}: f32 mode fused {e_gpu:.2e}, literal {e_lit:.2e} (float32 cpu {e_cpu:.2e}); fused - literal "
          f"{d_paths:.2e}; bf16 - f32: {d_gpu:.2e} (cpu chain {d_cpu:.2e}); relative to max-abs {scale:.3f}")
    assert e_gpu <= 4 * e_cpu
    assert d_paths <= 4 * e_cpu
    assert bool(torch.isfinite(out["bf16", True]).all()) and d_gpu <= 4 * d_cpu


# ---- the driver ----

@pytest.fixture(scope="module")
def weights_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("drunet") / "drunet_synthetic.pth")
    torch.save(synthetic_state_dict(seed=0), path)
    return path


COMMON = ["--device", "cuda", "--dataset", "synthetic", "--indices", "0,1", "--model_kind", "DiffPIR_DRUNet",
          "--diffpir_iterations", "4"]


def run_test_py(*flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), *COMMON, *flags], capture_output=True, text=True,
                          timeout=300)


@pytest.mark.parametrize("task", [["--task", "deblurring", "--kernel", "Gaussian_R2"], ["--task", "sr", "--sr_factor", "2"]])
def test_test_py_runs_the_diffpir_baseline(weights_file, task):
    r = run_test_py(*task, "--drunet_weights", weights_file)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert "N: 2" in lines
    assert math.isfinite(float([ln for ln in lines if ln.startswith("PSNR:")][0].split()[-1]))


def test_test_py_names_the_missing_flag():
    r = run_test_py("--task", "deblurring", "--kernel", "Gaussian_R2")
    assert r.returncode != 0 and "--drunet_weights" in r.stderr
