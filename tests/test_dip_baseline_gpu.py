"""GPU: the Deep Image Prior decoder kernels (sei_dip_*, through models.dip) and the baseline against a float64 torch
restatement of deepinv v0.2.0's ConvDecoder / DeepImagePrior, written out here as nn.Sequential and run on the CPU.

Bars. Relative L2 <= 1e-4 per tensor, the project's float32 bar: the float32 torch restatement against the float64 one gives
1.3e-7 on the loss and 1.9e-6 on the whole gradient at these shapes. The trajectory bar is measured inside the test: 10 times
the deviation of the float32 torch restatement from the float64 one over the same steps, with a floor of 1e-6 relative."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import _native as N
import physics
from models import get_model
from models.dip import ConvDecoderParams, DecoderPlan, DeepImagePrior, decoder_backward, decoder_forward, decoder_sizes
from test_dip_baseline import _args
from test_tv_baseline import blur_circ, gaussian_r2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-4


# ---- the float64 restatement -----------------------------------------------------------------------------------------

def oracle_decoder(img_shape, in_size=(16, 16), layers=7, channels=32, dtype=torch.float64):
    """deepinv v0.2.0's ConvDecoder: per stage Upsample(nearest) - Conv3x3 - ReLU - BatchNorm, one more Conv3x3 - ReLU -
    BatchNorm at the final size, a 1x1 head. Always in training mode."""
    mods = []
    for hw in decoder_sizes(img_shape[1:], in_size, layers):
        mods += [nn.Upsample(size=hw, mode="nearest"), nn.Conv2d(channels, channels, 3, 1, padding=1, bias=True), nn.ReLU(),
                 nn.BatchNorm2d(channels, affine=True)]
    mods += [nn.Conv2d(channels, channels, 3, 1, padding=1, bias=True), nn.ReLU(), nn.BatchNorm2d(channels, affine=True),
             nn.Conv2d(channels, img_shape[0], 1, 1, padding=0, bias=True)]
    return nn.Sequential(*mods).to(dtype).train()


def load_bucket(net, flat):
    """The flat bucket (module order) into the oracle's parameters."""
    pos = 0
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(flat[pos:pos + p.numel()].view(p.shape).to(p.dtype))
            pos += p.numel()
    assert pos == flat.numel()
    return net


def bucket_of(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors])


def rel(got, ref):
    got, ref = got.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    return float(torch.linalg.vector_norm(got - ref) / torch.linalg.vector_norm(ref))


def resample_matrices(H, W):
    from physics import _bands
    return tuple(torch.from_numpy(np.asarray(_bands.aa_bicubic_matrix(n, 1 / 2), dtype=np.float64)) for n in (H, W))


def operator(kind, H, W):
    """(the GPU physics or None for the identity, the float64 A on the CPU)."""
    if kind == "identity":
        return None, (lambda v: v)
    if kind == "blur":
        k = gaussian_r2()
        return physics.BlurV2(kernel=physics.get_kernel("Gaussian_R2")[None, None].cuda()), (lambda v: blur_circ(v, k))
    dv, dh = resample_matrices(H, W)
    return physics.Downsampling(rate=2, antialias=True), (lambda v: dv.to(v.dtype) @ v @ dh.to(v.dtype).T)


def random_bucket(params, seed):
    """torch's initialisation with every BatchNorm's gamma and beta moved off 1 and 0."""
    g = torch.Generator().manual_seed(seed)
    flat = params.flat.clone()
    stages, _ = params.views(flat)
    for st in stages:
        st["gamma"].copy_(0.5 + torch.rand(32, generator=g))
        st["beta"].copy_(torch.rand(32, generator=g) - 0.5)
    return flat


# ---- single kernels --------------------------------------------------------------------------------------------------

def stage_fwd(x_nchw, ss, w, bias, out_hw, gamma=None, beta=None):
    """sei_dip_stage_fwd on an NCHW (1, 32, h, w) input; returns (a NCHW, stats[128])."""
    hi, wi = x_nchw.shape[-2:]
    ho, wo = out_hw
    a_prev = x_nchw[0].permute(1, 2, 0).contiguous()
    gamma = torch.ones(32, device="cuda") if gamma is None else gamma
    beta = torch.zeros(32, device="cuda") if beta is None else beta
    a_out = torch.empty(ho * wo, 32, device="cuda")
    stats = torch.empty(128, device="cuda")
    work = torch.empty(N.lib().sei_dip_work_floats(ho, wo, 32, 3), device="cuda")
    N.call("sei_dip_stage_fwd", a_prev.data_ptr(), N.ptr(ss), w.data_ptr(), bias.data_ptr(), gamma.data_ptr(),
           beta.data_ptr(), a_out.data_ptr(), stats.data_ptr(), hi, wi, ho, wo, 32, 1e-5, work.data_ptr())
    return a_out.view(ho, wo, 32).permute(2, 0, 1)[None].contiguous(), stats


@pytest.mark.parametrize("hin,win,hout,wout", [(16, 26, 26, 41), (102, 3, 162, 7), (7, 1, 3, 5), (5, 16, 1, 26),
                                               (26, 102, 41, 162)])
def test_nearest_map_is_torch_s_exactly(hin, win, hout, wout):
    """An identity centre tap, zero bias and the identity in place of the incoming BatchNorm: the stage is
    relu(F.interpolate(x, mode="nearest")), bit for bit."""
    g = torch.Generator().manual_seed(hin * 1000 + wout)
    x = torch.randn((1, 32, hin, win), generator=g).cuda()
    w = torch.zeros(32, 32, 3, 3, device="cuda")
    w[torch.arange(32), torch.arange(32), 1, 1] = 1.0
    a, _ = stage_fwd(x, None, w, torch.zeros(32, device="cuda"), (hout, wout))
    want = F.relu(F.interpolate(x, size=(hout, wout), mode="nearest"))
    assert torch.equal(a, want)
    want_cpu = F.relu(F.interpolate(x.cpu(), size=(hout, wout), mode="nearest"))
    assert torch.equal(a.cpu(), want_cpu)


def test_padding_is_zero_behind_the_incoming_batch_norm():
    """One stage whose incoming BatchNorm has beta = 5: the halo contributes 0, not the shift. Also the stage's own channel
    statistics against float64 (the mean is large against the spread: a cancelling variance would show)."""
    g = torch.Generator().manual_seed(11)
    x = torch.rand((1, 32, 9, 13), generator=g, dtype=torch.float64)
    w = 0.1 * torch.randn((32, 32, 3, 3), generator=g, dtype=torch.float64)
    bias = torch.randn(32, generator=g, dtype=torch.float64) + 3.0
    scale = 0.5 + torch.rand(32, generator=g, dtype=torch.float64)
    shift = torch.full((32,), 5.0, dtype=torch.float64)
    gamma, beta = 0.5 + torch.rand(32, generator=g, dtype=torch.float64), torch.randn(32, generator=g, dtype=torch.float64)
    u = F.interpolate(x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), size=(14, 21), mode="nearest")
    ref = F.relu(F.conv2d(u, w, bias, padding=1))
    wrong = F.relu(F.conv2d(F.pad(u, (1, 1, 1, 1), value=5.0), w, bias))
    ss = torch.cat([scale, shift]).float().cuda()
    a, stats = stage_fwd(x.float().cuda(), ss, w.float().cuda(), bias.float().cuda(), (14, 21), gamma.float().cuda(),
                         beta.float().cuda())
    err = rel(a, ref)
    print(f"padding domain: rel {err:.2e}; a shift-filled halo would be off by {rel(wrong, ref):.2e}")
    assert rel(wrong, ref) > 1e-2 and err <= BAR
    mean, var = ref.mean(dim=(0, 2, 3)), ref.var(dim=(0, 2, 3), unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    want = torch.cat([mean, rstd, gamma * rstd, beta - mean * gamma * rstd])
    errs = [rel(stats[i * 32:(i + 1) * 32], want[i * 32:(i + 1) * 32]) for i in range(4)]
    print("stats (mean, rstd, scale, shift) rel:", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= BAR


@pytest.mark.parametrize("hin,win,hout,wout", [(7, 5, 11, 9), (9, 6, 6, 4), (1, 4, 5, 4), (16, 16, 19, 20)])
def test_data_gradient_is_the_adjoint_of_the_stage(hin, win, hout, wout):
    """BatchNorm frozen to a scale (shift 0, bias 0) and positive inputs and weights, so the ReLU is the identity and the stage
    is linear: <stage_bwd_data(g) * scale, x> = <g, stage_fwd(x)> to 1e-5, the dot products in float64."""
    g = torch.Generator().manual_seed(hin * 100 + hout)
    x = (0.1 + torch.rand((1, 32, hin, win), generator=g)).cuda()
    w = (0.01 + torch.rand((32, 32, 3, 3), generator=g)).cuda()
    scale = (0.5 + torch.rand(32, generator=g)).cuda()
    ss = torch.cat([scale, torch.zeros(32, device="cuda")])
    gout = torch.randn((1, 32, hout, wout), generator=g).cuda()
    a, _ = stage_fwd(x, ss, w, torch.zeros(32, device="cuda"), (hout, wout))
    assert float(a.min()) > 0
    g_cl = gout[0].permute(1, 2, 0).contiguous()
    g_prev = torch.empty(hin * win, 32, device="cuda")
    N.call("sei_dip_stage_bwd_data", g_cl.data_ptr(), w.data_ptr(), g_prev.data_ptr(), hin, win, hout, wout, 32)
    gx = g_prev.view(hin, win, 32).permute(2, 0, 1)[None] * scale.view(1, -1, 1, 1)
    lhs = float((gx.double() * x.double()).sum())
    rhs = float((gout.double() * a.double()).sum())
    print(f"adjoint {hin}x{win} -> {hout}x{wout}: {lhs:.9e} vs {rhs:.9e}")
    assert abs(lhs - rhs) <= 1e-5 * abs(rhs)


# ---- the whole decoder -----------------------------------------------------------------------------------------------

CASES = [
    ((3, 40, 56), (16, 16), 7, "identity"),                     # non-square, no multiple of any tile
    ((3, 12, 20), (16, 16), 7, "identity"),                     # shrinking extents
    ((3, 9, 13), (4, 4), 3, "identity"),
    ((3, 1, 5), (4, 4), 2, "identity"),                         # a one-pixel extent
    ((3, 40, 56), (16, 16), 7, "blur"),
    ((3, 40, 56), (16, 16), 7, "sr"),
]


@pytest.mark.parametrize("img_shape,in_size,layers,kind", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_decoder_forward_loss_and_gradients_match_float64(img_shape, in_size, layers, kind):
    C, H, W = img_shape
    torch.manual_seed(H * 100 + W)
    params = ConvDecoderParams(img_shape, in_size, layers)
    flat = random_bucket(params, seed=layers)
    g = torch.Generator().manual_seed(5)
    z = torch.randn((1, 32) + tuple(in_size), generator=g)
    op, A64 = operator(kind, H, W)
    y = torch.rand(tuple(A64(torch.zeros((1, C, H, W), dtype=torch.float64)).shape), generator=g, dtype=torch.float64)

    net = load_bucket(oracle_decoder(img_shape, in_size, layers), flat)
    ref_x = net(z.double())
    ref_loss = ((A64(ref_x) - y) ** 2).mean()
    ref_grads = torch.autograd.grad(ref_loss, list(net.parameters()))

    plan = DecoderPlan(params, "cuda")
    flat_d = flat.cuda()
    x_hat = decoder_forward(plan, flat_d, z.cuda())
    assert x_hat.shape == (1, C, H, W)
    xr = x_hat.clone().requires_grad_(True)                      # the loss and the physics transpose, through autograd
    loss = (((xr if op is None else op.A(xr)) - y.float().cuda()) ** 2).mean()
    (g_x,) = torch.autograd.grad(loss, xr)
    grads = decoder_backward(plan, flat_d, g_x)
    errs = {"x_hat": rel(x_hat, ref_x), "loss": abs(float(loss) - float(ref_loss)) / float(ref_loss)}
    stages, head = params.views(grads)
    names = [f"{l}.{k}" for l in range(layers) for k in ("w", "b", "gamma", "beta")] + ["head.w", "head.b"]
    tensors = [st[k] for st in stages for k in ("w", "b", "gamma", "beta")] + [head["w"], head["b"]]
    assert len(tensors) == len(ref_grads)
    for name, got, want in zip(names, tensors, ref_grads):
        assert got.shape == want.shape
        errs[name] = rel(got, want)
    errs["all gradients"] = rel(grads, bucket_of(ref_grads))
    worst = max(errs, key=errs.get)
    print(f"decoder {img_shape} {kind}: x_hat {errs['x_hat']:.2e}, loss {errs['loss']:.2e}, gradient "
          f"{errs['all gradients']:.2e}, worst {worst} {errs[worst]:.2e}")
    assert errs[worst] <= BAR, errs


# ---- the fit ---------------------------------------------------------------------------------------------------------

def torch_trajectory(img_shape, flat, z, y, A, steps, dtype):
    """`steps` iterations of torch.optim.Adam(lr 5e-3) on mean((A(G(z)) - y)^2) on the CPU; the loss of every step."""
    net = load_bucket(oracle_decoder(img_shape, dtype=dtype), flat)
    opt = torch.optim.Adam(net.parameters(), lr=5e-3)
    z, y, losses = z.to(dtype), y.to(dtype), []
    for _ in range(steps):
        opt.zero_grad()
        loss = ((A(net(z)) - y) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    return np.array(losses)


def seeded_start(seed, img_shape):
    """What DeepImagePrior.forward draws under torch.manual_seed(seed): the bucket from the CPU generator, z from the
    device's."""
    torch.manual_seed(seed)
    params = ConvDecoderParams(img_shape)
    z = torch.randn([32, 16, 16], device="cuda")[None]
    return params.flat.clone(), z.cpu()


def measurement(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def deviation(losses, ref):
    return float(np.max(np.abs(np.asarray(losses) - ref) / ref))


def test_trajectory_follows_float64_adam():
    """20 iterations at 40 x 56, deblurring, from the same bucket and code: the loss of every step."""
    op, A64 = operator("blur", 40, 56)
    y = measurement((1, 3, 40, 56), seed=21)
    flat, z = seeded_start(4, (3, 40, 56))
    ref = torch_trajectory((3, 40, 56), flat, z, y, A64, 20, torch.float64)
    dev32 = deviation(torch_trajectory((3, 40, 56), flat, z, y, A64, 20, torch.float32), ref)
    model = DeepImagePrior(op, iterations=20, trace=True)
    torch.manual_seed(4)
    model(y.float().cuda())
    dev = deviation(model.loss_history, ref)
    bar = max(10 * dev32, 1e-6)
    print(f"trajectory: float32 torch deviates by {dev32:.2e}, the kernels by {dev:.2e} (bar {bar:.2e}); "
          f"loss {ref[0]:.5f} -> {ref[-1]:.5f}")
    assert model.iterations_run == 20 and len(model.loss_history) == 20
    assert dev <= bar


def test_graph_replay_and_eager_give_the_same_bits():
    op, _ = operator("blur", 40, 56)
    y = measurement((1, 3, 40, 56), seed=22).float().cuda()
    runs = []
    for graph in (True, False, True):
        model = DeepImagePrior(op, iterations=12, graph=graph, trace=True)
        torch.manual_seed(6)
        x_hat = model(y)
        runs.append((x_hat, model.final_weights, model.last_loss, model.loss_history))
    for other in runs[1:]:                                       # replay == eager, and two runs from the same seeds
        assert torch.equal(runs[0][0], other[0]) and torch.equal(runs[0][1], other[1])
        assert runs[0][2] == other[2] and runs[0][3] == other[3]
    assert math.isfinite(runs[0][2])


@pytest.mark.parametrize("task", ["deblurring", "sr"])
def test_through_the_factory(task):
    flags = ["--task", "deblurring", "--kernel", "Gaussian_R2"] if task == "deblurring" else ["--task", "sr", "--sr_factor", "2"]
    args = _args("--model_kind", "DeepImagePrior", *flags, dip_iterations=40)
    n = 32 if task == "deblurring" else 16
    op, A64 = operator("blur" if task == "deblurring" else "sr", 32, 32)
    y = measurement((1, 3, n, n), seed=23)
    model = get_model(args, physics=op, device="cuda")
    torch.manual_seed(0)
    x_hat = model(y.float().cuda())
    dip = model.get_backbone()
    assert x_hat.shape == (1, 3, 32, 32) and dip.iterations_run == 40 and len(model.get_weights()) == 0
    flat, z = seeded_start(0, (3, 32, 32))
    ref = torch_trajectory((3, 32, 32), flat, z, y, A64, 40, torch.float64)
    l32 = torch_trajectory((3, 32, 32), flat, z, y, A64, 40, torch.float32)
    bar = max(10 * abs(l32[-1] - ref[-1]) / ref[-1], 1e-6)
    dev = abs(dip.last_loss - ref[-1]) / ref[-1]
    print(f"factory {task}: loss {ref[0]:.5f} -> {dip.last_loss:.5f} (float64 {ref[-1]:.5f}): rel {dev:.2e}, bar {bar:.2e}")
    assert dip.last_loss < ref[0]
    first = get_model(_args("--model_kind", "DeepImagePrior", *flags, dip_iterations=1), physics=op, device="cuda")
    torch.manual_seed(0)
    first(y.float().cuda())
    assert dip.last_loss < first.get_backbone().last_loss       # below the loss of iteration 1
    assert dev <= bar
    with pytest.raises(ValueError, match="one measurement"):
        model(torch.rand(2, 3, n, n, device="cuda"))
    if task == "deblurring":                                     # A's output does not match y: both shapes are named
        wrong = DeepImagePrior(op, sr_factor=2, iterations=2)
        with pytest.raises(ValueError, match=r"64, 64.*32, 32"):
            wrong(y.float().cuda())


COMMON = ["--device", "cuda", "--dataset", "synthetic", "--indices", "0"]


def run_test_py(*flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), *COMMON, *flags], capture_output=True, text=True,
                          timeout=300)


@pytest.mark.parametrize("task", [["--task", "deblurring", "--kernel", "Gaussian_R2"], ["--task", "sr", "--sr_factor", "2"]])
def test_test_py_runs_the_dip_baseline(task):
    r = run_test_py(*task, "--model_kind", "DeepImagePrior", "--dip_iterations", "25")
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert "N: 1" in lines
    assert math.isfinite(float([ln for ln in lines if ln.startswith("PSNR:")][0].split()[-1]))


def test_test_py_no_longer_refuses_the_dip_switch():
    r = run_test_py("--task", "deblurring", "--kernel", "Gaussian_R2", "--model_kind", "dip")
    assert r.returncode != 0 and "Unknown model kind" in r.stderr and "outside the hot path" not in r.stderr
