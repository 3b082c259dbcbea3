"""GPU: the sei_drunet_* kernels one by one against float64 F.conv2d with a derived accumulation bound, the DRUNet of
models/drunet.py in both arithmetic modes against the float64 restatement of tests/drunet_ref.py, the PlugAndPlay baseline
against pnp_ref, determinism and batch independence, and test.py --model_kind PlugAndPlay end to end."""
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
from drunet_ref import assert_activation_range, forward_ref, pnp_ref, synthetic_state_dict
from models.drunet import DRUNet
from models.pnp import PnPModel
from test_tv_baseline import blur_circ, gaussian_r2, piecewise_constant_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, U16 = 2.0 ** -24, 2.0 ** -8        # float32 unit roundoff; the issue's allowance for a bf16 result
GUARD_FILL = 3.0


def bf16_values(shape, seed, scale=1.0, signed=True):
    """float64 values that bfloat16 holds exactly."""
    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(shape, generator=g) if signed else torch.rand(shape, generator=g)) * scale
    return t.to(torch.bfloat16).double()


def to_grid(x):
    """NCHW float64 (bf16-exact) -> the kernel's grid on the GPU: (guard + B (H+2) (W+2) + guard, C) bfloat16 with a zero
    border and guard rows pre-filled with GUARD_FILL. Returns (whole buffer, guard rows)."""
    B, C, H, W = x.shape
    guard = W + 3
    body = F.pad(x.permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1)).reshape(-1, C)
    buf = torch.full((body.shape[0] + 2 * guard, C), GUARD_FILL, dtype=torch.float64)
    buf[guard:guard + body.shape[0]] = body
    return buf.to(torch.bfloat16).cuda(), guard


def empty_grid(B, C, H, W, dtype):
    guard = W + 3 if dtype == torch.bfloat16 else 0
    rows = B * (H + 2) * (W + 2)
    buf = torch.zeros((rows + 2 * guard, C), dtype=dtype)
    if guard:
        buf[:guard] = GUARD_FILL
        buf[-guard:] = GUARD_FILL
    return buf.cuda(), guard


def from_grid(buf, guard, B, C, H, W):
    """(interior as NCHW float64, True when the border is all zero and the guard rows still hold GUARD_FILL)."""
    rows = B * (H + 2) * (W + 2)
    t = buf.cpu().double()
    body = t[guard:guard + rows].view(B, H + 2, W + 2, C)
    border = body.clone()
    border[:, 1:-1, 1:-1] = 0
    clean = float(border.abs().max()) == 0.0
    if guard:
        clean = clean and bool((t[:guard] == GUARD_FILL).all()) and bool((t[-guard:] == GUARD_FILL).all())
    return body[:, 1:-1, 1:-1].permute(0, 3, 1, 2).contiguous(), clean


def trunk_grid(t):
    """NCHW float64 -> the float32 trunk on grid rows (border zero)."""
    return F.pad(t.permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1)).reshape(-1, t.shape[1]).float().cuda()


def pack(w):
    """(Cout, Cin, kh, kw) -> tap-major (Cout, kh kw Cin) bfloat16 on the GPU."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).to(torch.bfloat16).contiguous().cuda()


def check(name, got, ref, bound):
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: max |err| {float(err.max()):.3e}, max err / bound {worst:.3f}")
    assert bool((err <= bound).all()), (name, worst)


@pytest.mark.parametrize("B,H,W", [(1, 4, 5), (2, 9, 13), (1, 32, 40)])
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_conv3x3_both_epilogues(C, B, H, W):
    """42, 330 and 1428 grid rows: below one tile, not a tile multiple, several tiles. Operands are bf16-exact, so the only
    error is the float32 accumulation: |err| <= 9 Cin 2^-24 conv(|x|, |w|), plus 2^-23 (|T_in| + |T_skip|) for the two float32
    additions of epilogue 1, plus 2^-8 |ref| for a bf16 result."""
    x = bf16_values((B, C, H, W), C + H)
    w = bf16_values((C, C, 3, 3), C + W, scale=math.sqrt(2.0 / (9 * C)))
    t_in, t_skip = bf16_values((B, C, H, W), 3), bf16_values((B, C, H, W), 4)
    conv = F.conv2d(x, w, padding=1)
    acc_bound = 9 * C * U32 * F.conv2d(x.abs(), w.abs(), padding=1)
    xg, guard = to_grid(x)
    wt = pack(w)
    # epilogue 0
    yg, _ = empty_grid(B, C, H, W, torch.bfloat16)
    N.call("sei_drunet_conv3x3", xg[guard:].data_ptr(), wt.data_ptr(), C, C, B, H, W, 0, None, None, None,
           yg[guard:].data_ptr())
    got, clean = from_grid(yg, guard, B, C, H, W)
    ref = conv.relu()
    check(f"conv3x3 relu C={C} {B}x{H}x{W}", got, ref, acc_bound + U16 * ref.abs())
    assert clean
    # epilogue 1, without and with the second addend
    for skip in (None, t_skip):
        yg, _ = empty_grid(B, C, H, W, torch.bfloat16)
        tg, _ = empty_grid(B, C, H, W, torch.float32)
        tin = trunk_grid(t_in)
        N.call("sei_drunet_conv3x3", xg[guard:].data_ptr(), wt.data_ptr(), C, C, B, H, W, 1, tin.data_ptr(),
               None if skip is None else trunk_grid(skip).data_ptr(), tg.data_ptr(), yg[guard:].data_ptr())
        ref = t_in + conv + (0 if skip is None else skip)
        bound = acc_bound + 2 * U32 * (t_in.abs() + (0 if skip is None else skip.abs()) + conv.abs())
        got32, clean32 = from_grid(tg, 0, B, C, H, W)
        got16, clean16 = from_grid(yg, guard, B, C, H, W)
        tag = f"conv3x3 residual{'+skip' if skip is not None else ''} C={C} {B}x{H}x{W}"
        check(tag + " f32", got32, ref, bound)
        check(tag + " bf16", got16, ref, bound + U16 * ref.abs())
        assert clean32 and clean16
    # the input grid was only read
    _, clean = from_grid(xg, guard, B, C, H, W)
    assert clean
    # every tile of sei_drunet_conv3x3_ex gives the bits of the default one (yg, tg: the last call above)
    for pb in (1, 2, 4):
        y2, _ = empty_grid(B, C, H, W, torch.bfloat16)
        t2, _ = empty_grid(B, C, H, W, torch.float32)
        N.call("sei_drunet_conv3x3_ex", xg[guard:].data_ptr(), wt.data_ptr(), C, C, B, H, W, 1, tin.data_ptr(),
               trunk_grid(t_skip).data_ptr(), t2.data_ptr(), y2[guard:].data_ptr(), pb)
        assert torch.equal(t2, tg) and torch.equal(y2, yg), pb


@pytest.mark.parametrize("B,H,W", [(2, 8, 12), (1, 6, 10)])
@pytest.mark.parametrize("Clo,Chi", [(64, 128), (256, 512)])
def test_down_and_up(Clo, Chi, B, H, W):
    """nn.Conv2d(Clo, Chi, 2, 2) from (H, W) to (H/2, W/2) and nn.ConvTranspose2d(Chi, Clo, 2, 2) back up."""
    x = bf16_values((B, Clo, H, W), Clo + H)
    w = bf16_values((Chi, Clo, 2, 2), 5, scale=math.sqrt(1.0 / (4 * Clo)))
    ref = F.conv2d(x, w, stride=2)
    bound = 4 * Clo * U32 * F.conv2d(x.abs(), w.abs(), stride=2)
    xg, guard = to_grid(x)
    h, wd = H // 2, W // 2
    yg, g2 = empty_grid(B, Chi, h, wd, torch.bfloat16)
    tg, _ = empty_grid(B, Chi, h, wd, torch.float32)
    N.call("sei_drunet_down", xg[guard:].data_ptr(), pack(w).data_ptr(), Clo, Chi, B, h, wd, tg.data_ptr(), yg[g2:].data_ptr())
    got32, c32 = from_grid(tg, 0, B, Chi, h, wd)
    got16, c16 = from_grid(yg, g2, B, Chi, h, wd)
    check(f"down {Clo}->{Chi} {B}x{H}x{W} f32", got32, ref, bound)
    check(f"down {Clo}->{Chi} {B}x{H}x{W} bf16", got16, ref, bound + U16 * ref.abs())
    assert c32 and c16

    z = bf16_values((B, Chi, h, wd), Chi + W)
    wu = bf16_values((Chi, Clo, 2, 2), 6, scale=math.sqrt(1.0 / Chi))
    ref = F.conv_transpose2d(z, wu, stride=2)
    bound = Chi * U32 * F.conv_transpose2d(z.abs(), wu.abs(), stride=2)
    zg, g2 = to_grid(z)
    wt = wu.permute(2, 3, 1, 0).reshape(4 * Clo, Chi).to(torch.bfloat16).contiguous().cuda()
    yg, guard = empty_grid(B, Clo, H, W, torch.bfloat16)
    tg, _ = empty_grid(B, Clo, H, W, torch.float32)
    N.call("sei_drunet_up", zg[g2:].data_ptr(), wt.data_ptr(), Chi, Clo, B, h, wd, tg.data_ptr(), yg[guard:].data_ptr())
    got32, c32 = from_grid(tg, 0, B, Clo, H, W)
    got16, c16 = from_grid(yg, guard, B, Clo, H, W)
    check(f"up {Chi}->{Clo} {B}x{H}x{W} f32", got32, ref, bound)
    check(f"up {Chi}->{Clo} {B}x{H}x{W} bf16", got16, ref, bound + U16 * ref.abs())
    assert c32 and c16


def test_head_and_tail():
    """(2, 9, 13), sigma 0.05. The head rounds its inputs to bf16 like every convolution input, so the reference takes the
    bf16-exact image and bf16(sigma); its K is 9 x 4 (the 28 padding channels add exact zeros)."""
    B, H, W, C = 2, 9, 13, 64
    x = bf16_values((B, 3, H, W), 21, signed=False)
    sigma = float(torch.tensor(0.05).to(torch.bfloat16))
    w = bf16_values((C, 4, 3, 3), 22, scale=math.sqrt(1.0 / 36))
    x0 = torch.cat([x, torch.full((B, 1, H, W), sigma, dtype=torch.float64)], 1)
    ref = F.conv2d(x0, w, padding=1)
    bound = 36 * U32 * F.conv2d(x0.abs(), w.abs(), padding=1)
    wt = pack(F.pad(w, (0, 0, 0, 0, 0, 28)))
    yg, guard = empty_grid(B, C, H, W, torch.bfloat16)
    tg, _ = empty_grid(B, C, H, W, torch.float32)
    nbytes = N.lib().sei_drunet_work_bytes(B, H, W)
    assert nbytes == (B * (H + 2) * (W + 2) + 2 * (W + 3)) * 32 * 2
    work = torch.full((nbytes,), 0x7F, dtype=torch.uint8, device="cuda")
    N.call("sei_drunet_head", x.float().cuda().data_ptr(), 0.05, wt.data_ptr(), C, B, H, W, tg.data_ptr(),
           yg[guard:].data_ptr(), work.data_ptr())
    got32, c32 = from_grid(tg, 0, B, C, H, W)
    got16, c16 = from_grid(yg, guard, B, C, H, W)
    check("head f32", got32, ref, bound)
    check("head bf16", got16, ref, bound + U16 * ref.abs())
    assert c32 and c16

    z = bf16_values((B, C, H, W), 23)
    wt3 = bf16_values((3, C, 3, 3), 24, scale=math.sqrt(1.0 / (9 * C)))
    ref = F.conv2d(z, wt3, padding=1)
    bound = 9 * C * U32 * F.conv2d(z.abs(), wt3.abs(), padding=1)
    zg, guard = to_grid(z)
    out = torch.full((B, 3, H, W), 9.0, device="cuda")
    N.call("sei_drunet_tail", zg[guard:].data_ptr(), pack(F.pad(wt3, (0, 0, 0, 0, 0, 0, 0, 13))).data_ptr(), C, B, H, W,
           out.data_ptr())
    check("tail", out.cpu().double(), ref, bound)


# ---- the network ----

def image(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def nets():
    """{nb: (state dict, DRUNet on the GPU)} at full widths."""
    out = {}
    for nb in (1, 4):
        sd = synthetic_state_dict(nb=nb, seed=nb)
        net = DRUNet(nb=nb)
        net.load_state_dict(sd)
        out[nb] = (sd, net.cuda().eval())
    return out


@pytest.mark.parametrize("nb,shape", [(4, (2, 3, 32, 40)), (1, (1, 3, 20, 27)), (1, (1, 3, 68, 75)), (1, (1, 3, 40, 56))])
def test_network_matches_float64_restatement(nets, nb, shape):
    """Max-norm error relative to the float64 output's max-abs: the f32 mode at most 4x that of the float32 CPU chain, the
    bf16 mode at most 4x that of the float32 CPU chain with its weights and convolution inputs rounded to bf16 (another
    accumulation order, another realisation of the same roundings). Both modes give the same bits on a second run."""
    sd, net = nets[nb]
    x, sigma = image(shape, seed=shape[-1]), 0.05
    if shape[-2] % 8 == 0 and shape[-1] % 8 == 0:
        assert_activation_range(sd, x, sigma)
    ref = forward_ref(sd, x, sigma, torch.float64)
    scale = float(ref.abs().max())
    e_cpu32 = float((forward_ref(sd, x, sigma, torch.float32).double() - ref).abs().max()) / scale
    e_cpu16 = float((forward_ref(sd, x, sigma, torch.float32, round_bf16=True).double() - ref).abs().max()) / scale
    errs = {}
    for mode in ("f32", "bf16"):
        net.compute_dtype = mode
        got = net(x.cuda(), sigma)
        again = net(x.cuda(), sigma)
        assert got.shape == x.shape and got.dtype == torch.float32 and torch.equal(got, again)
        errs[mode] = float((got.cpu().double() - ref).abs().max()) / scale
    net.compute_dtype = "bf16"
    print(f"DRUNet nb={nb} {shape}: f32 mode {errs['f32']:.2e} (float32 cpu {e_cpu32:.2e}), bf16 mode {errs['bf16']:.2e} "
          f"(bf16-rounded cpu {e_cpu16:.2e}), relative to max-abs {scale:.3f}")
    assert errs["f32"] <= 4 * e_cpu32
    assert errs["bf16"] <= 4 * e_cpu16


def test_network_is_batch_independent(nets):
    sd, net = nets[1]
    x = image((3, 3, 40, 56), seed=7).cuda()
    for mode in ("bf16", "f32"):
        net.compute_dtype = mode
        whole = net(x, 0.1)
        for i in (0, 2):
            assert torch.equal(net(x[i:i + 1].contiguous(), 0.1)[0], whole[i]), (mode, i)
    net.compute_dtype = "bf16"
    with pytest.raises(TypeError):
        net(x.double(), 0.1)


# ---- PlugAndPlay ----

def _pnp_case(kind):
    if kind == "deblurring":
        _, y = piecewise_constant_case()                      # 40 x 56, Gaussian_R2
        k = gaussian_r2()
        op = physics.BlurV2(kernel=physics.get_kernel("Gaussian_R2")[None, None].cuda())
        A = lambda dt: (lambda v: blur_circ(v, k.to(dt)))                       # noqa: E731
        At = lambda dt: (lambda v: blur_circ(v, k.to(dt), transpose=True))      # noqa: E731
        return y, op, A, At
    from physics import _bands
    op = physics.Downsampling(rate=2, antialias=True)
    y = torch.rand((1, 3, 16, 20), generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    dv, dh = (torch.from_numpy(np.asarray(_bands.aa_bicubic_matrix(n, 1 / 2), dtype=np.float64)) for n in (32, 40))
    uv, uh = (torch.from_numpy(np.asarray(_bands.plain_bicubic_matrix(n, 2), dtype=np.float64)) for n in (16, 20))
    A = lambda dt: (lambda v: dv.to(dt) @ v @ dh.to(dt).T)                      # noqa: E731
    At = lambda dt: (lambda v: uv.to(dt) @ v @ uh.to(dt).T)                     # noqa: E731  (the reference's adjoint)
    return y, op, A, At


@pytest.mark.parametrize("kind", ["deblurring", "sr"])
def test_pnp_matches_float64_restatement(nets, kind):
    """f32 mode, nb = 1, cg_tol = 0 and cg_max_iter = 12 so that both sides run the same iteration counts: the error against
    float64 is at most 4x that of the float32 CPU chain. The default bf16 mode stays within 4x the distance that rounding
    to bf16 moves the float32 CPU chain, and is finite."""
    sd, net = nets[1]
    y, op, A, At = _pnp_case(kind)
    s = 5 / 255
    kw = dict(cg_max_iter=12, cg_tol=0.0)
    ref, ran = pnp_ref(y, A(torch.float64), At(torch.float64), sd, s, torch.float64, **kw)
    cpu32, _ = pnp_ref(y, A(torch.float32), At(torch.float32), sd, s, torch.float32, **kw)
    cpu16, _ = pnp_ref(y, A(torch.float32), At(torch.float32), sd, s, torch.float32, round_bf16=True, **kw)
    scale = float(ref.abs().max())
    model = PnPModel(op, s, net, **kw)
    assert len(model.state_dict()) == 0
    out = {}
    for mode in ("f32", "bf16"):
        net.compute_dtype = mode
        out[mode] = model(y.float().cuda()).cpu().double()
        assert model.iterations_run == ran == 8 and out[mode].shape == ref.shape
    net.compute_dtype = "bf16"
    e_gpu = float((out["f32"] - ref).abs().max()) / scale
    e_cpu = float((cpu32.double() - ref).abs().max()) / scale
    d_gpu = float((out["bf16"] - out["f32"]).abs().max()) / scale
    d_cpu = float((cpu16.double() - cpu32.double()).abs().max()) / scale
    print(f"PnP {kind}: f32 mode {e_gpu:.2e} (float32 cpu {e_cpu:.2e}); bf16 - f32: {d_gpu:.2e} (cpu chain {d_cpu:.2e}); "
          f"relative to max-abs {scale:.3f}")
    assert e_gpu <= 4 * e_cpu
    assert bool(torch.isfinite(out["bf16"]).all()) and d_gpu <= 4 * d_cpu


@pytest.fixture(scope="module")
def weights_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("drunet") / "drunet_synthetic.pth")
    torch.save(synthetic_state_dict(seed=0), path)
    return path


COMMON = ["--device", "cuda", "--dataset", "synthetic", "--indices", "0,1", "--model_kind", "PlugAndPlay"]


def run_test_py(*flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), *COMMON, *flags], capture_output=True, text=True,
                          timeout=300)


@pytest.mark.parametrize("task", [["--task", "deblurring", "--kernel", "Gaussian_R2"], ["--task", "sr", "--sr_factor", "2"]])
def test_test_py_runs_the_pnp_baseline(weights_file, task):
    r = run_test_py(*task, "--drunet_weights", weights_file)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert "N: 2" in lines
    assert math.isfinite(float([ln for ln in lines if ln.startswith("PSNR:")][0].split()[-1]))


def test_test_py_names_the_missing_flag():
    r = run_test_py("--task", "deblurring", "--kernel", "Gaussian_R2")
    assert r.returncode != 0 and "--drunet_weights" in r.stderr
