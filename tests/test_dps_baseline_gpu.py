"""GPU: sei_drunet_conv3x3_masked and the sei_dps_* kernels one by one against float64, the DRUNet's vector-Jacobian product
in both arithmetic modes against the float64 transposed network of tests/dps_ref.py under the device's own ReLU masks, its
onesplit path, the DPS baseline against dps_ref around a stub denoiser and around the DRUNet, and test.py --model_kind DPS
end to end."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import _native as N
import physics
from dps_ref import dps_ref, dps_step_ref, mask_flips, masked_denoiser_ref, preactivation_signs_ref, tables_ref, vjp_ref
from drunet_ref import assert_activation_range, synthetic_state_dict
from models.dps import DPS
from models.drunet import DRUNet, onesplit_plan
from test_pnp_baseline_gpu import U32, _pnp_case, bf16_values, check, empty_grid, from_grid, pack, to_grid
from test_tv_baseline import blur_circ, gaussian_r2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rand64(shape, seed, normal=False):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn if normal else torch.rand)(shape, generator=g, dtype=torch.float64)


def rel(a, b, scale):
    return float((a.double().cpu() - b.double().cpu()).abs().max()) / scale


# ---- the new kernels ----

@pytest.mark.parametrize("B,H,W", [(2, 8, 12), (1, 9, 7)])
@pytest.mark.parametrize("C", [64, 128])
def test_masked_conv3x3(C, B, H, W):
    """280 and 99 grid rows: several tiles, not a tile multiple. Operands are bf16-exact, so the only error is the float32
    accumulation, |err| <= 9 Cin 2^-24 conv(|x|, |w|) (test_pnp_baseline_gpu.py::test_conv3x3_both_epilogues), plus one
    bf16 ulp of the result; where the mask is not above zero the result is exactly 0. The mask holds zeros, negative zeros,
    negative values and the smallest positive bf16."""
    x = bf16_values((B, C, H, W), C + H)
    w = bf16_values((C, C, 3, 3), C + W, scale=math.sqrt(2.0 / (9 * C)))
    mid = bf16_values((B, C, H, W), 9).clamp_min(0)                      # a ReLU output: about half zeros
    mid[:, :, 0, 0] = -0.0
    mid[:, :, 0, 1] = -1.5
    mid[:, :, 1, 0] = 2.0 ** -133                                         # the least bf16 above zero
    conv = F.conv2d(x, w, padding=1)
    ref = conv * (mid > 0)
    ulp = torch.where(ref != 0, 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(1e-300))) - 7), torch.zeros_like(ref))
    bound = (9 * C * U32 * F.conv2d(x.abs(), w.abs(), padding=1) + ulp) * (mid > 0)
    xg, guard = to_grid(x)
    mg, _ = to_grid(mid)
    assert bool(((mg[guard:guard + B * (H + 2) * (W + 2)].view(B, H + 2, W + 2, C)[:, 1:-1, 1:-1].cpu() > 0) ==
                 (mid > 0).permute(0, 2, 3, 1)).all())
    wt = pack(w)
    yg, _ = empty_grid(B, C, H, W, torch.bfloat16)
    N.call("sei_drunet_conv3x3_masked", xg[guard:].data_ptr(), wt.data_ptr(), C, C, B, H, W, mg[guard:].data_ptr(),
           yg[guard:].data_ptr())
    got, clean = from_grid(yg, guard, B, C, H, W)
    check(f"masked conv3x3 C={C} {B}x{H}x{W}", got, ref, bound)
    assert clean and 0.2 < float((mid > 0).double().mean()) < 0.8
    for grid, values in ((xg, x), (mg, mid)):                             # the inputs were only read
        back, clean = from_grid(grid, guard, B, C, H, W)
        assert clean and torch.equal(back, values)
    for pb in (1, 2, 4):                                                  # every tile gives the bits of the default one
        y2, _ = empty_grid(B, C, H, W, torch.bfloat16)
        N.call("sei_drunet_conv3x3_masked_ex", xg[guard:].data_ptr(), wt.data_ptr(), C, C, B, H, W, mg[guard:].data_ptr(),
               y2[guard:].data_ptr(), pb)
        assert torch.equal(y2, yg), pb


DPS_SHAPES = [(3, 105), (3, 4653), (1, 7), (2, 1026)]          # images of m floats: m % 4 of 1, 1, 3, 2; 4653: five workgroups


def _out_values(B, m, seed):
    """Denoiser outputs around [0, 1] with values exactly at 0 and 1 (inside the inclusive mask) and just outside."""
    o = rand64((B, m), seed) * 1.5 - 0.25
    o[:, 0], o[:, 1], o[:, 2], o[:, 3] = 0.0, 1.0, -2.0 ** -20, 1 + 2.0 ** -20
    return o.float()


@pytest.mark.parametrize("B,m", DPS_SHAPES)
def test_dps_u_and_seed_kernels(B, m):
    """u = clamp(2 o - 1, -1, 1) / 2 + 0.5: two roundings (the subtraction and the last addition), |err| <= 2^-24 (|2 o - 1| +
    1). The seed is a selection: the bits of A^T r where -1 <= 2 o - 1 <= 1 in float32, zero elsewhere."""
    o = _out_values(B, m, seed=m)
    atr = rand64((B, m), m + 1, normal=True).float()
    u, seed = torch.empty((B, m), device="cuda"), torch.empty((B, m), device="cuda")
    od, atrd = o.cuda(), atr.cuda()
    N.call("sei_dps_u", od.data_ptr(), u.data_ptr(), B, m)
    N.call("sei_dps_seed", atrd.data_ptr(), od.data_ptr(), seed.data_ptr(), B, m)
    t = 2 * o.double() - 1
    check(f"dps u {B}x{m}", u.cpu().double(), t.clamp(-1, 1) / 2 + 0.5, U32 * (t.abs() + 1))
    inside = (t >= -1) & (t <= 1)
    assert bool(inside[:, 0].all()) and bool(inside[:, 1].all()) and not bool(inside[:, 2].any()) and not bool(inside[:, 3].any())
    assert torch.equal(seed.cpu(), torch.where(inside, atr, torch.zeros_like(atr)))
    assert 0 < int(inside.sum()) < inside.numel()


@pytest.mark.parametrize("B,m", DPS_SHAPES)
def test_dps_residual_kernel(B, m):
    """r = Au - y is one rounding. f_b adds m squares in float32: whatever the order, |err| <= (m + 4) 2^-24 f_b (m - 1
    additions, the square, r's own rounding twice, the halving exact); s_b = 1 / (2 sqrt(f_b)) halves that relative error
    and adds three roundings. The last image has Au = y: r = 0, f = 0 and s = 0 exactly. Same bits on a second run and for
    an image alone."""
    Au, y = rand64((B, m), m + 2).float(), rand64((B, m), m + 3).float()
    y[-1] = Au[-1]
    r, f, s = torch.empty((B, m), device="cuda"), torch.full((B,), -1.0, device="cuda"), torch.full((B,), -1.0, device="cuda")
    part = torch.empty(N.lib().sei_dps_partials(B, m), device="cuda")
    args = lambda a, b, rr, ff, ss, nb: (a.data_ptr(), b.data_ptr(), rr.data_ptr(), part.data_ptr(), ff.data_ptr(),   # noqa: E731
                                        ss.data_ptr(), nb, m)
    Ad, yd = Au.cuda(), y.cuda()
    N.call("sei_dps_residual", *args(Ad, yd, r, f, s, B))
    r64 = Au.double() - y.double()
    f64 = 0.5 * (r64 * r64).sum(1)
    check(f"dps residual {B}x{m}", r.cpu().double(), r64, U32 * r64.abs())
    check(f"dps f {B}x{m}", f.cpu().double(), f64, (m + 4) * U32 * f64)
    assert float(f[-1]) == 0.0 and float(s[-1]) == 0.0 and float(r[-1].abs().max()) == 0.0
    if B > 1:
        s64 = 1 / (2 * f64[:-1].sqrt())
        check(f"dps s {B}x{m}", s.cpu().double()[:-1], s64, (0.5 * (m + 4) + 3) * U32 * s64)
        assert bool((f64[:-1] > 0).all())
    r2, f2, s2 = torch.empty_like(r), torch.empty_like(f), torch.empty_like(s)
    N.call("sei_dps_residual", *args(Ad, yd, r2, f2, s2, B))
    assert torch.equal(r2, r) and torch.equal(f2, f) and torch.equal(s2, s)
    for b in range(B):                                   # (image b alone starts 16-byte aligned only in a copy of its own)
        ab, yb = Ad[b].clone(), yd[b].clone()
        N.call("sei_dps_residual", *args(ab, yb, r2, f2, s2, 1))
        assert torch.equal(r2[0], r[b]) and torch.equal(f2[0], f[b]) and torch.equal(s2[0], s[b]), b


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("B,m", DPS_SHAPES)
def test_dps_step_kernel(B, m, last):
    """x = ((c0 x0 + st nz) + c1 x) - (ginv s_b) g with x0 = clamp(2 o - 1, -1, 1): no operand passes through more than five
    roundings, so |err| <= 5 2^-24 (|c0 x0| + |st nz| + |c1 x| + |ginv s_b g|) =: e; xin = x / den + 0.5 adds two roundings,
    |err| <= e / den + 2^-24 (|x| / den + |xin|). The scalars are the float32 values the kernel is handed. One s_b is 0."""
    _, ac = tables_ref()
    at, an = (float(ac[1]), 1.0) if last else (float(ac[501]), float(ac[301]))
    st = math.sqrt((1 - at / an) * (1 - an) / (1 - at))
    c2 = math.sqrt(max((1 - an) - st * st, 0.0))
    c0, c1, ginv, den = (float(np.float32(v)) for v in (math.sqrt(an) - c2 * math.sqrt(at) / math.sqrt(1 - at),
                                                        c2 / math.sqrt(1 - at), 1 / (2 * math.sqrt(at)), 2 * math.sqrt(an)))
    st = float(np.float32(st))
    o = _out_values(B, m, seed=m + 4)
    g, nz, x = (rand64((B, m), m + 5 + i, normal=True).float() for i in range(3))
    s = (rand64((B,), m + 8) + 0.5).float()
    s[-1] = 0.0
    xd, xin = x.cuda(), torch.empty((B, m), device="cuda")
    od, gd, nzd, sd = o.cuda(), g.cuda(), nz.cuda(), s.cuda()
    N.call("sei_dps_step", od.data_ptr(), gd.data_ptr(), nzd.data_ptr(), sd.data_ptr(), xd.data_ptr(), xin.data_ptr(), c0, c1,
           st, ginv, den, B, m)
    x0 = (2 * o.double() - 1).clamp(-1, 1)
    terms = [c0 * x0, st * nz.double(), c1 * x.double(), (ginv * s.double())[:, None] * g.double()]
    ref = terms[0] + terms[1] + terms[2] - terms[3]
    e = 5 * U32 * sum(t.abs() for t in terms)
    check(f"dps step {B}x{m} x", xd.cpu().double(), ref, e)
    check(f"dps step {B}x{m} xin", xin.cpu().double(), ref / den + 0.5, e / den + U32 * (ref.abs() / den + (ref / den + 0.5).abs()))
    assert bool(torch.isfinite(xd).all()) and bool(torch.isfinite(xin).all())
    if last:
        assert st == 0.0 and c1 == 0.0 and c0 == 1.0 and den == 2.0


# ---- the vector-Jacobian product ----

def _net(nb, seed):
    sd = synthetic_state_dict(nb=nb, seed=seed)
    net = DRUNet(nb=nb)
    net.load_state_dict(sd)
    return sd, net.cuda().eval()


@pytest.fixture(scope="module")
def net2():
    """Full widths, nb = 2 (a stage's first and last block differ), x of (2, 3, 32, 40) (H != W), sigma 0.05."""
    sd, net = _net(2, 2)
    x = torch.rand((2, 3, 32, 40), generator=torch.Generator().manual_seed(40))
    g = torch.randn((2, 3, 32, 40), generator=torch.Generator().manual_seed(41))
    assert_activation_range(sd, x, 0.05)
    return sd, net, x, g, preactivation_signs_ref(sd, x.double(), 0.05, torch.float64)


@pytest.fixture(scope="module")
def net1():
    return _net(1, 1)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_vjp_matches_float64_under_the_device_masks(net2, mode):
    """With the ReLUs fixed to tape.masks() the VJP is a linear map and float64 gives its exact value (the flip of one
    near-zero pre-activation would move the result by far more than float32 rounding). Max-norm error relative to the
    float64 result's max-abs: the f32 mode at most 4x that of the float32 CPU chain under the same masks, the bf16 mode at
    most 4x that of the float32 CPU chain with weights and every transposed convolution's input rounded to bf16. The
    masks themselves differ from the float64 forward's signs in at most 4x as many units as the CPU chain's, plus 8.
    Same bits on a second run and for image 0 alone."""
    sd, net, x, g, signs64 = net2
    net.compute_dtype = mode
    try:
        xd, gd = x.cuda(), g.cuda()
        out, tape = net.forward_taped(xd, 0.05)
        assert torch.equal(out, net(xd, 0.05))
        masks = [m.cpu() for m in tape.masks()]
        assert [tuple(m.shape) for m in masks] == [tuple(s.shape) for s in signs64] and masks[0].dtype == torch.bool
        gx = net.vjp(tape, gd)
        assert gx.shape == x.shape and gx.dtype == torch.float32
        out2, tape2 = net.forward_taped(xd, 0.05)
        assert torch.equal(out2, out) and torch.equal(net.vjp(tape2, gd), gx)
        out0, tape0 = net.forward_taped(xd[:1].contiguous(), 0.05)
        assert torch.equal(out0[0], out[0]) and torch.equal(net.vjp(tape0, gd[:1].contiguous())[0], gx[0])
    finally:
        net.compute_dtype = "bf16"
    rounded = mode == "bf16"
    ref = vjp_ref(sd, masks, g.double(), torch.float64)
    scale = float(ref.abs().max())
    e_gpu = rel(gx, ref, scale)
    e_cpu = rel(vjp_ref(sd, masks, g, torch.float32, round_bf16=rounded), ref, scale)
    n_gpu = mask_flips(masks, signs64)
    n_cpu = mask_flips(preactivation_signs_ref(sd, x, 0.05, torch.float32, round_bf16=rounded), signs64)
    print(f"DRUNet VJP {mode}: {e_gpu:.2e} (cpu chain {e_cpu:.2e}) relative to max-abs {scale:.3f}; mask flips against float64: "
          f"device {n_gpu}, cpu chain {n_cpu}, of {sum(m.numel() for m in masks)} units")
    assert e_gpu <= 4 * e_cpu
    assert n_gpu <= 4 * n_cpu + 8


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_vjp_onesplit_is_the_adjoint_of_the_gather(net1, mode):
    """(1, 3, 68, 75) runs as four 64 x 64 corner pieces: vjp equals the hand-made composition of the direct VJP over the
    pieces, bit for bit (the kernels give the same bits at every batch position and the pieces are summed in the plan's
    order). Below 32 forward_taped raises."""
    sd, net = net1
    net.compute_dtype = mode
    try:
        x, g = rand64((1, 3, 68, 75), 75).float().cuda(), rand64((1, 3, 68, 75), 76, normal=True).float().cuda()
        out, tape = net.forward_taped(x, 0.05)
        assert torch.equal(out, net(x, 0.05)) and tape.masks()[0].shape == (4, 64, 64, 64)
        gx = net.vjp(tape, g)
        want = torch.zeros_like(g)
        for pr, pc, orow, ocol, irow, icol in onesplit_plan(68, 75):
            _, piece_tape = net.forward_taped(x[..., pr, pc].contiguous(), 0.05)
            gp = torch.zeros((1, 3, 64, 64), device="cuda")
            gp[..., irow, icol] = g[..., orow, ocol]
            want[..., pr, pc] += net.vjp(piece_tape, gp)
        assert torch.equal(gx, want) and float(gx.abs().max()) > 0
        with pytest.raises(ValueError, match="replicate"):
            net.forward_taped(x[..., :24, :40].contiguous(), 0.05)
        with pytest.raises(ValueError):
            net.vjp(tape, g[..., :64, :64].contiguous())
    finally:
        net.compute_dtype = "bf16"


# ---- DPS ----

GAIN = 1.0


def stub_gain(s):
    return GAIN / (1.0 + s)


class StubDenoiser:
    """D(v, s) = blur_circ(v, k) * gain(s) in torch on the GPU, with the taped interface."""

    def __init__(self):
        self.k = gaussian_r2().float().cuda()

    def forward_taped(self, v, sigma):
        return blur_circ(v, self.k) * stub_gain(sigma), sigma

    def vjp(self, tape, g):
        return blur_circ(g, self.k, transpose=True) * stub_gain(tape)


def stub_ref(dtype):
    k = gaussian_r2().to(dtype)
    return lambda v, s: blur_circ(v, k) * stub_gain(s)


def _dps_case(kind, B):
    y, op, A, At = _pnp_case(kind)
    y = torch.cat([y] + [(y + 0.05 * rand64(y.shape, 20 + b, normal=True)) for b in range(1, B)], 0)
    return y, op, A, tuple(At(torch.float64)(y).shape)


def _fixed(draws):
    class Fixed(DPS):
        def draw(self, i, like):
            return draws[i].float().to(like.device)
    return Fixed


@pytest.mark.parametrize("kind", ["deblurring", "sr"])
def test_dps_with_a_stub_denoiser_matches_float64(kind):
    """max_iter = 5, B = 2, the same noise on both sides. The fused path is within 4x the float32 CPU chain's error against
    float64, and the literal path agrees with the fused one to the same bar. The float64 run meets the conditions that make
    the comparison meaningful: every f_b > 0, no |2 out - 1| within 1e-6 of 1, and some but not all pixels clamped."""
    y, op, A, x_shape = _dps_case(kind, 2)
    draws = {i: rand64(x_shape, 200 + i, normal=True) for i in range(6)}
    stats = {}
    ref = dps_ref(y, A(torch.float64), stub_ref(torch.float64), draws, 5, torch.float64, stats=stats)
    cpu32 = dps_ref(y.float(), A(torch.float32), stub_ref(torch.float32), draws, 5, torch.float32)
    share = stats["clamped"] / stats["pixels"]
    print(f"DPS stub {kind}: f_b in [{min(stats['f']):.3e}, {max(stats['f']):.3e}], least distance of |2 out - 1| from 1 "
          f"{stats['edge']:.2e}, clamped share {share:.3f}")
    assert len(stats["f"]) == 10 and min(stats["f"]) > 0 and stats["edge"] > 1e-6 and 0 < share < 1
    scale = float(ref.abs().max())
    out = {}
    for fused in (True, False):
        model = _fixed(draws)(op, StubDenoiser(), max_iter=5, fused=fused)
        out[fused] = model(y.float().cuda())
        assert out[fused].shape == ref.shape and len(model.state_dict()) == 0
    e_gpu, e_lit, e_cpu = rel(out[True], ref, scale), rel(out[False], ref, scale), rel(cpu32, ref, scale)
    d_paths = rel(out[True], out[False], scale)
    print(f"DPS stub {kind}: fused {e_gpu:.2e}, literal {e_lit:.2e} (float32 cpu {e_cpu:.2e}); fused - literal {d_paths:.2e}; "
          f"relative to max-abs {scale:.3f}")
    assert e_gpu <= 4 * e_cpu
    assert d_paths <= 4 * e_cpu


class Recorder:
    """The DRUNet with the masks of every taped forward kept."""

    def __init__(self, net):
        self.net, self.masks = net, []

    def forward_taped(self, v, sigma):
        out, tape = self.net.forward_taped(v, sigma)
        self.masks.append([m.cpu() for m in tape.masks()])
        return out, tape

    def vjp(self, tape, g):
        return self.net.vjp(tape, g)


def test_dps_with_the_drunet(net1):
    """nb = 1, max_iter = 2, deblurring at 32 x 40: the output is finite, has the image's shape and the same bits on a second
    run with the same noise. One step, (500, 0), from a given x agrees with the restatement when the restatement's denoiser
    is the network under the device's masks: in f32 mode within 4x the float32 CPU chain's error against float64; in bf16
    mode the distance from float64 is within 4x the distance by which rounding weights and convolution inputs to bf16 (in
    the forward and in the transposed network) moves the float32 CPU chain under the same masks."""
    sd, net = net1
    k = gaussian_r2()
    op = physics.BlurV2(kernel=physics.get_kernel("Gaussian_R2")[None, None].cuda())
    A = lambda dt: (lambda v: blur_circ(v, k.to(dt)))                       # noqa: E731
    x_true = rand64((1, 3, 32, 40), 50)
    y = blur_circ(x_true, k) + 0.02 * rand64(x_true.shape, 51, normal=True)
    draws = {i: rand64(x_true.shape, 300 + i, normal=True) for i in range(3)}
    _, ac = tables_ref()
    at, an = float(ac[501]), float(ac[1])
    try:
        for mode in ("bf16", "f32"):
            net.compute_dtype = mode
            model = _fixed(draws)(op, net, max_iter=2)
            out = model(y.float().cuda())
            assert out.shape == x_true.shape and bool(torch.isfinite(out).all()) and torch.equal(model(y.float().cuda()), out)
            rec = Recorder(net)
            model = _fixed(draws)(op, rec, max_iter=2)
            assert model.pairs == [(500, 0), (0, -1)]
            model.pairs = model.pairs[:1]                                  # one step: what comes back is the next aux
            got = model(y.float().cuda())
            masks = rec.masks[0]

            def step(dtype, rounded):
                D = masked_denoiser_ref(sd, masks, dtype, rounded)
                nxt = dps_step_ref(draws[0].to(dtype), y.to(dtype), A(dtype), D, draws[1].to(dtype), at, an)
                return nxt / (2 * math.sqrt(an)) + 0.5

            ref, cpu32 = step(torch.float64, False), step(torch.float32, False)
            scale = float(ref.abs().max())
            e_gpu, e_cpu = rel(got, ref, scale), rel(cpu32, ref, scale)
            if mode == "f32":
                print(f"DPS step f32: {e_gpu:.2e} (float32 cpu {e_cpu:.2e}) relative to max-abs {scale:.3f}")
                assert e_gpu <= 4 * e_cpu
            else:
                d_cpu = rel(step(torch.float32, True), cpu32, scale)
                print(f"DPS step bf16: {e_gpu:.2e} from float64 (bf16 rounding moves the cpu chain by {d_cpu:.2e}) relative to "
                      f"max-abs {scale:.3f}")
                assert e_gpu <= 4 * d_cpu
    finally:
        net.compute_dtype = "bf16"


# ---- the driver ----

@pytest.fixture(scope="module")
def weights_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("drunet") / "drunet_synthetic.pth")
    torch.save(synthetic_state_dict(seed=0), path)
    return path


COMMON = ["--device", "cuda", "--dataset", "synthetic", "--indices", "0", "--model_kind", "DPS", "--dps_iterations", "2"]


def run_test_py(*flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), *COMMON, *flags], capture_output=True, text=True,
                          timeout=300)


@pytest.mark.parametrize("task", [["--task", "deblurring", "--kernel", "Gaussian_R2"], ["--task", "sr", "--sr_factor", "2"]])
def test_test_py_runs_the_dps_baseline(weights_file, task):
    r = run_test_py(*task, "--drunet_weights", weights_file)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert "N: 1" in lines
    assert math.isfinite(float([ln for ln in lines if ln.startswith("PSNR:")][0].split()[-1]))


def test_test_py_names_the_missing_flag():
    r = run_test_py("--task", "deblurring", "--kernel", "Gaussian_R2")
    assert r.returncode != 0 and "--drunet_weights" in r.stderr
