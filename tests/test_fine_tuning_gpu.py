"""Fine-tuning on measurements on the GPU: sei_sgd_fused through optim.FlatSGD against the reference's own values (g17)
and a float64 restatement, its loop shapes, determinism, frozen ranges, the literal torch sequence, the captured step and
train.py --fine_tuning end to end (reference: demo/train.py:95-114, 144-186, 245-264).

Bars. Parameters: 1e-6 of max |p| in max-norm (five float32 roundings of quantities bounded by max |p|; the fixture keeps
lr |g'| <= max |p|). Penalty: max(2 |ref32 - ref64|, 1e-6 ref64), the reference's own float32 loop setting the margin and
the floor covering three roundings per positive term plus a double accumulation. Captured step: the bars of
tests/test_loss_gpu.py::test_graphed_step_matches_eager. Every test prints its figures before it asserts (pytest -s)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fine_tuning_common as ft

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARAM_BAR = 1e-6          # of max |p|, max-norm: five float32 roundings of quantities bounded by max |p|


def _fill(model, values=None, grads=None):
    """Write per-name values into the parameters / the gradient bucket (both are views of the flat buckets)."""
    with torch.no_grad():
        for name, p in model.named_parameters():
            if values is not None:
                p.copy_(torch.as_tensor(np.asarray(values[name])).to(p.device))
            if grads is not None:
                p._sei_grad_view.copy_(torch.as_tensor(np.asarray(grads[name])).to(p.device))


def _random_like(model, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return {n: scale * torch.randn(p.shape, generator=gen) for n, p in model.named_parameters()}


def _check_params(backbone, want64, what):
    got = backbone.flat_params.detach().cpu().double()
    err = float((got - want64).abs().max() / want64.abs().max())
    print(f"{what}: parameters max-norm error {err:.2e} of max |p| (bar {PARAM_BAR:.0e})")
    assert err <= PARAM_BAR, (what, err)


def _check_penalty(opt, ref32, ref64, what):
    got = float(opt.last_penalty)
    bar = ft.penalty_bar(ref32, ref64)
    print(f"{what}: penalty {got:.9e} vs float64 {ref64:.9e} (error {abs(got - ref64):.2e}, float32 reference error "
          f"{abs(float(ref32) - ref64):.2e}, bar {bar:.2e})")
    assert opt.last_penalty.dim() == 0 and opt.last_penalty.is_cuda and opt.last_penalty.dtype == torch.float32
    assert abs(got - ref64) <= bar, (what, got, ref64, bar)


def _torch_penalty32(anchor_values, current_values):
    """The torch WeightsDistanceLoss in float32 on the CPU: the float32 comparand where no fixture holds one."""
    from losses.weights_distance_loss import WeightsDistanceLoss
    flat = lambda values: {n.replace(".", "_"): torch.as_tensor(np.asarray(v)) for n, v in values.items()}
    shapes = {n: tuple(v.shape) for n, v in flat(anchor_values).items()}
    a, m = ft.Bucket(shapes, flat(anchor_values)), ft.Bucket(shapes, flat(current_values))
    return float(WeightsDistanceLoss(pretrained_model=a, lambd=1, device="cpu")(m).detach())


def test_kernel_against_g17(golden):
    from optim import FlatSGD
    g = golden("g17_weights_distance")
    model = ft.Bucket(ft.G17_SHAPES, ft.g17_values(g, "anchor")).to("cuda")
    model.compute_dtype = "bf16"                              # the step then writes the bf16 copy as well
    opt = FlatSGD(model, lr=float(g["lr"]), anchor=True, lambd=1)
    _fill(model, ft.g17_values(g, "param"), ft.g17_values(g, "grad"))
    grads_before = model.flat_grads.clone()
    opt.step()
    torch.cuda.synchronize()
    _check_params(model, ft.per_element(model, ft.g17_values(g, "f64.stepped")), "g17")
    _check_penalty(opt, float(g["loss32"]), float(g["loss64"]), "g17")
    pad = ft.padding_mask(model).cuda()
    assert pad.sum() == 192 - 135 + 63 + 63
    assert not model.flat_params[pad].any() and not model.flat_grads[pad].any()
    assert not model.flat_shadow[pad].view(torch.int16).any()
    assert torch.equal(model.flat_grads, grads_before)
    assert torch.equal(model.flat_shadow.view(torch.int16), model.flat_params.to(torch.bfloat16).view(torch.int16))
    from models import _ops
    assert _ops.plain_shadow_is_current(model)


LOOP_SHAPES = {"a": (9250,), "c": (7,)}
GRID_CAP = 2          # workgroups: 2 x 256 threads x two quads = 4,096 elements per trip of the grid-stride loop


@pytest.mark.parametrize("only,cap", [(["a"], GRID_CAP), (["c"], 0), (None, GRID_CAP), (None, 0)])
def test_loop_shapes(only, cap):
    """`a` alone is one range of 9,280 elements = 2 x 4,096 + 1,088: with the grid capped at 2 workgroups that is two
    two-quad trips and then a single-quad tail for 272 of the 512 threads (the others have run out); `c` alone is one
    range of exactly 64 elements, a quarter of one wave. The whole bucket (9,344) under the cap and under the library's
    own grid (5 workgroups, one trip) give the same figures."""
    import _native as N
    from optim import FlatSGD
    anchors = {n: 0.5 * v for n, v in _random_like(ft.Bucket(LOOP_SHAPES), 41).items()}
    model = ft.Bucket(LOOP_SHAPES, anchors).to("cuda")
    model.compute_dtype = "bf16"
    opt = FlatSGD(model, lr=1e-2, anchor=True, lambd=1, only=only, grid_cap=cap)
    # (parameters outside `only` stay on their anchors, as frozen ones do; their gradients are non-zero all the same)
    current = {n: anchors[n] + (0.1 * v if only is None or n in only else 0) for n, v in _random_like(model, 42).items()}
    grads = _random_like(model, 43)
    _fill(model, current, grads)
    from models import _ops
    _ops.refresh_plain_shadow(model)
    ranges = None if only is None else [(getattr(model, n)._sei_bucket_offset,
                                         getattr(model, n)._sei_bucket_offset + (getattr(model, n).numel() + 63) // 64 * 64)
                                        for n in only]
    if only == ["a"]:
        assert ranges == [(0, 9280)] and N.lib().sei_sgd_partials(0, 9280, cap) == 2
    if only == ["c"]:
        assert ranges == [(9280, 9344)]
    p64 = model.flat_params.detach().cpu().double()
    shadow_before = model.flat_shadow.clone()
    want, ref64 = ft.restated_step(p64, ft.per_element(model, grads), ft.per_element(model, anchors),
                                   ft.coefficients(model), 1e-2, ranges)
    ref32 = _torch_penalty32(anchors, current)
    opt.step()
    torch.cuda.synchronize()
    what = f"only={only} cap={cap}"
    _check_params(model, want, what)
    _check_penalty(opt, ref32, ref64, what)
    pad = ft.padding_mask(model).cuda()
    assert not model.flat_params[pad].any() and not model.flat_shadow[pad].view(torch.int16).any()
    moved = torch.zeros(9344, dtype=torch.bool)
    for lo, hi in ranges or [(0, 9344)]:
        moved[lo:hi] = True
    moved = moved.cuda()
    assert torch.equal(model.flat_params.cpu().double()[~moved.cpu()], p64[~moved.cpu()])
    assert torch.equal(model.flat_shadow[~moved].view(torch.int16), shadow_before[~moved].view(torch.int16))
    assert torch.equal(model.flat_shadow[moved].view(torch.int16),
                       model.flat_params[moved].to(torch.bfloat16).view(torch.int16))


def _g17_run(golden, anchor, mode="f32"):
    from optim import FlatSGD
    g = golden("g17_weights_distance")
    model = ft.Bucket(ft.G17_SHAPES, ft.g17_values(g, "anchor")).to("cuda")
    model.compute_dtype = mode
    opt = FlatSGD(model, lr=float(g["lr"]), anchor=anchor, lambd=1)
    return g, model, opt


def test_first_step_at_the_anchor(golden):
    """d = 0 everywhere: the penalty is exactly zero and the step is plain SGD's, bit for bit."""
    outs = []
    for anchor in (True, None):
        g, model, opt = _g17_run(golden, anchor, "bf16")
        _fill(model, None, ft.g17_values(g, "grad"))
        opt.step()
        torch.cuda.synchronize()
        assert float(opt.last_penalty) == 0.0
        outs.append((model.flat_params.clone(), model.flat_shadow.clone()))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert torch.equal(outs[0][1].view(torch.int16), outs[1][1].view(torch.int16))
    p0 = ft.per_element(model, ft.g17_values(g, "anchor"))
    want = p0 - float(g["lr"]) * ft.per_element(model, ft.g17_values(g, "grad"))
    _check_params(model, want, "plain SGD")
    assert not torch.equal(outs[1][0].cpu().double(), p0)


def test_two_runs_give_the_same_bits(golden):
    outs = []
    for _ in range(2):
        g, model, opt = _g17_run(golden, True)
        _fill(model, ft.g17_values(g, "param"), ft.g17_values(g, "grad"))
        opt.step()
        opt.step()                                            # (the second from the moved weights, same gradients)
        torch.cuda.synchronize()
        outs.append((model.flat_params.clone(), opt.last_penalty.clone()))
    assert float(outs[0][1]) > 0
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))


def test_frozen_ranges():
    """only = the conv_last pair of a nested model: nothing outside their two ranges changes, float32 or bf16, with
    non-zero gradients everywhere; inside they move as the restatement says; and since a frozen parameter sits on its
    anchor, the penalty over the two ranges is the penalty over the whole bucket."""
    from models import _ops
    from optim import FlatSGD
    keys = ["model.model.conv_last.weight", "model.model.conv_last.bias"]
    model = ft.Nested(seed=3).to("cuda")
    bb = model.get_backbone()
    bb.compute_dtype = "bf16"
    anchors = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    opt = FlatSGD(model, lr=1e-2, anchor=True, lambd=1, only=keys)
    whole = FlatSGD(model, lr=0.0, anchor=True, lambd=1)      # same anchor; lr = 0: reads the penalty, moves nothing
    current = dict(anchors)
    for k, v in _random_like(model, 44, 0.1).items():
        if k in keys:
            current[k] = anchors[k] + v
    grads = _random_like(model, 45)
    _fill(model, current, grads)
    assert all(bool((p._sei_grad_view != 0).all()) for p in model.parameters())
    _ops.refresh_plain_shadow(bb)
    p_before, s_before = bb.flat_params.clone(), bb.flat_shadow.clone()
    whole.step()
    assert torch.equal(bb.flat_params.view(torch.int32), p_before.view(torch.int32))
    full_penalty = whole.last_penalty.clone()
    ranges = opt._ranges
    assert len(ranges) == 2 and all(lo % 64 == 0 and hi % 64 == 0 for lo, hi in ranges)
    want, ref64 = ft.restated_step(p_before.cpu().double(), ft.per_element(model, grads), ft.per_element(model, anchors),
                                   ft.coefficients(model), 1e-2, ranges)
    opt.step()
    torch.cuda.synchronize()
    inside = torch.zeros(bb.flat_params.numel(), dtype=torch.bool, device="cuda")
    for lo, hi in ranges:
        inside[lo:hi] = True
    assert torch.equal(bb.flat_params[~inside].view(torch.int32), p_before[~inside].view(torch.int32))
    assert torch.equal(bb.flat_shadow[~inside].view(torch.int16), s_before[~inside].view(torch.int16))
    for k in keys:
        assert not torch.equal(model.get_parameter(k).detach().cpu(), current[k])
    _check_params(bb, want, "frozen ranges")
    assert torch.equal(bb.flat_shadow[inside].view(torch.int16), bb.flat_params[inside].to(torch.bfloat16).view(torch.int16))
    ref32 = _torch_penalty32(anchors, current)
    _check_penalty(opt, ref32, ref64, "frozen ranges")
    _check_penalty(whole, ref32, ref64, "whole bucket")
    # (double accumulation of the same non-zero terms, grouped differently, rounded to float32 once)
    print(f"penalty over the two ranges {float(opt.last_penalty):.9e}, over the whole bucket {float(full_penalty):.9e}")
    assert abs(float(opt.last_penalty) - float(full_penalty)) <= 1e-6 * ref64


def _small_unet(seed=0):
    import bench
    import models
    import physics
    args = bench.reference_args("cuda", hidden=8, scales=3)
    p = physics.get_physics(args, "cuda")
    torch.manual_seed(seed)
    model = models.get_model(args, p, "cuda").to("cuda")
    return args, p, model


def test_against_the_literal_path():
    """Three steps of FlatSGD against torch.optim.SGD on the same external gradients plus the autograd gradients of the
    torch WeightsDistanceLoss (lambd = 100 so that the penalty's share of the step is visible beside the gradients)."""
    from losses.weights_distance_loss import WeightsDistanceLoss
    from optim import FlatSGD
    lambd, lr = 100.0, 1e-2
    _, _, fused = _small_unet()
    _, _, literal = _small_unet()
    fb, lb = fused.get_backbone(), literal.get_backbone()
    assert torch.equal(fb.flat_params, lb.flat_params)
    opt = FlatSGD(fused, lr=lr, anchor=True, lambd=lambd)
    wd = WeightsDistanceLoss(pretrained_model=literal, lambd=lambd, device="cuda")
    sgd = torch.optim.SGD(literal.parameters(), lr=lr)
    pad = ft.padding_mask(fused).cuda()
    for step in range(3):
        g = torch.randn(fb.flat_grads.shape, generator=torch.Generator().manual_seed(50 + step)).cuda()
        g[pad] = 0
        fb.flat_grads.copy_(g)
        lb.flat_grads.copy_(g)
        value = wd(literal)
        penalty_grads = torch.autograd.grad(value, list(literal.parameters()))
        for p, pg in zip(literal.parameters(), penalty_grads):
            p.grad = p._sei_grad_view + pg
        sgd.step()
        opt.step()
        torch.cuda.synchronize()
        scale = float(lb.flat_params.abs().max())
        err = float((fb.flat_params - lb.flat_params).abs().max()) / scale
        pen = abs(float(opt.last_penalty) - float(value)) / max(float(value), 1e-30)
        print(f"step {step}: fused vs literal parameters {err:.2e} of max |p| = {scale:.3f}; penalty {float(opt.last_penalty):.6e} "
              f"vs {float(value):.6e} (rel {pen:.1e})")
        assert err <= PARAM_BAR, (step, err)
        if step == 0:
            assert float(opt.last_penalty) == 0.0 == float(value)
    assert float(opt.last_penalty) > 0


def test_captured_step_with_flat_sgd_matches_eager():
    """GraphedLossStep + FlatSGD.step() against zero_grad + loss + backward + FlatSGD.step() with the step's draws injected,
    two steps, at the bars the replay-against-eager tests of FlatAdam apply in float32. First step, same weights on both
    sides (tests/test_loss_gpu.py::test_graphed_step_matches_eager): loss to 1e-6 relative, the gradient bucket to 1e-5 of
    its largest entry -- the float atomics' arrival order; the weights after it then differ by at most lr times that, plus
    the step's own rounding (1e-6 of max |p|). Second step, from weights that differ by that much
    (test_graphed_training_tracks_eager_training's bar for every step after the first): loss, gradient norm and weights
    to 2e-3 relative."""
    from graphs import GraphedLossStep
    from losses import get_loss
    from losses.sure import embed_probe
    from optim import FlatSGD
    B = 4
    gen = torch.Generator().manual_seed(5)
    x = torch.rand((B, 3, 256, 256), generator=gen).cuda()
    draws = {"b": embed_probe(torch.empty(B, 3, 48, 48, device="cuda"), torch.randn((B, 3, 36, 36), generator=gen).cuda(), 6),
             "rate": torch.tensor([0.75, 0.5, 0.5, 0.75]).cuda(),
             "center": (2 * torch.rand((B, 2), generator=gen) - 1).cuda().view(B, 1, 1, 2),
             "noise": torch.randn((B, 3, 48, 48), generator=gen).cuda()}
    runs = {}
    for mode in ("eager", "graph"):
        args, p, model = _small_unet()
        bb = model.get_backbone()
        lf = get_loss(args, p)
        torch.cuda.manual_seed(7)
        y = p(x)
        opt = FlatSGD(model, lr=1e-2, anchor=True, lambd=1)
        graphed = GraphedLossStep(lf, model, opt, (B, 3, 48, 48), fuse_optimizer=False) if mode == "graph" else None
        hist = []
        for step in range(2):
            torch.manual_seed(30 + step)                      # CPU generator: the crop offsets
            if graphed is not None:
                bb.flat_grads.fill_(float("nan"))
                val = graphed(x, y, draws=draws)
            else:
                opt.zero_grad()
                val = lf(x=x, y=y, model=model, draws=draws)
                val.backward()
            grads = bb.flat_grads.clone()
            opt.step()
            torch.cuda.synchronize()
            hist.append((float(val.detach()), grads, bb.flat_params.clone(), float(opt.last_penalty)))
        runs[mode] = hist
    for step, ((le, ge, pe, ne), (lg, gg, pg, ng)) in enumerate(zip(runs["eager"], runs["graph"])):
        assert np.isfinite(le) and np.isfinite(lg) and torch.isfinite(gg).all()
        gerr = float((ge - gg).abs().max() / ge.abs().max())
        perr = float((pe - pg).abs().max() / pe.abs().max())
        print(f"step {step}: loss {lg:.8e} (graph) vs {le:.8e} (eager); gradients {gerr:.1e}; weights {perr:.1e}; "
              f"penalty {ng:.6e} vs {ne:.6e}")
        if step == 0:
            assert abs(le - lg) <= 1e-6 * abs(le), (le, lg)
            assert gerr < 1e-5, gerr
            assert float((pe - pg).abs().max()) <= 1e-2 * 1e-5 * float(ge.abs().max()) + PARAM_BAR * float(pe.abs().max())
        else:
            assert abs(le - lg) <= 2e-3 * abs(le), (le, lg)
            assert abs(float(ge.norm()) - float(gg.norm())) <= 2e-3 * float(ge.norm())
            assert perr < 2e-3, perr
    assert runs["graph"][0][3] == 0.0 == runs["eager"][0][3] and runs["graph"][1][3] > 0
    assert not torch.equal(runs["graph"][0][2], runs["graph"][1][2])


def test_train_script_fine_tuning(tmp_path):
    """train.py --fine_tuning --weights_distance_loss on a folder of three measured PNGs, from saved weights: the first
    step replays a hipGraph, the defaults are SGD at 1e-2, the logged losses are finite and the weights move."""
    from PIL import Image
    folder = tmp_path / "measurements"
    folder.mkdir()
    rng = np.random.default_rng(0)
    for k in range(3):
        Image.fromarray(rng.integers(0, 256, size=(64, 64, 3), dtype=np.uint8)).save(folder / f"y{k}.png")
    _, _, model = _small_unet()
    start = {k: v.detach().cpu().clone() for k, v in model.get_weights().items()}
    torch.save(start, tmp_path / "start.pt")
    out = tmp_path / "run"
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--device", "cuda", "--task", "deblurring", "--kernel",
           "Gaussian_R2", "--ProposedModel__architecture", "Convolutional", "--ConvolutionalModel__hidden_channels",
           "8", "--ConvolutionalModel__scales", "3", "--dataset", str(folder), "--PrepareTrainingPairs__crop_size", "64",
           "--batch_size", "2", "--epochs", "2", "--method", "proposed", "--fine_tuning", "--weights_distance_loss",
           # (two epochs: the default delayed_linear_decay divides by epochs // 2 - 1, in the reference as here)
           "--lr_scheduler_kind", "multi_step_decay",
           "--weights", str(tmp_path / "start.pt"), "--out_dir", str(out)]
    env = dict(os.environ, SEI_TRACE_STEP_KIND="1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "step kind: hipGraph replay" in r.stdout, r.stdout
    assert "Selected learning rate: 1.000000e-02" in r.stdout and "Selected optimizer: SGD" in r.stdout, r.stdout
    rows = open(out / "training.csv").read().strip().splitlines()
    assert rows[0] == "Epoch,Training Loss" and len(rows) == 3
    assert all(np.isfinite(float(r_.split(",")[1])) for r_ in rows[1:])
    w = torch.load(out / "weights.pt", map_location="cpu")
    assert set(w) == set(start) and any(not torch.equal(w[k], start[k]) for k in start)
    ckp = torch.load(out / "checkpoints" / "ckp_2.pt", map_location="cpu")
    assert ckp["optimizer"]["state"] == {} and ckp["optimizer"]["param_groups"][0]["momentum"] == 0
    # the Convolutional architecture has no conv_last: refused by name before anything runs
    r = subprocess.run(cmd[:-1] + [str(tmp_path / "run2"), "--fine_tuning_params"], capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode != 0 and "conv_last" in r.stderr, r.stdout + r.stderr
