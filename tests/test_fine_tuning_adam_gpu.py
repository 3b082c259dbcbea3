"""Fine-tuning with Adam on the GPU: sei_adam_anchor_fused against the float64 Adam model of tests/adam_ref.py fed the
restated penalised gradient, its bit identities with sei_adam_fused, its loop shapes and edges, optim.FlatAdam with frozen
ranges, the literal torch sequence, the captured step and train.py --fine_tuning --optimizer Adam end to end (reference:
demo/train.py:95-114, 144-186, 245-264).

Bars. Stages: adam_ref's derived ones, per element (4 u (|m| + S), 8 u (b2 v + (1 - b2) S^2), u |p| + 8 u |delta_k|), with
g' = grad_scale g + (2 c) d restated in numpy float32 in the kernel's documented order and handed to the model as its
gradient at grad_scale 1. Penalty: fine_tuning_common.penalty_bar against the float64 sum of c d^2. Literal path: the fused
step's max-norm error against a float64 run may be at most twice the literal float32 sequence's own, both in units of
max |p| (two float32 evaluation orders of one formula; the factor is the CT-filter test's margin over torch.matmul).
Captured step: the bars of tests/test_fine_tuning_gpu.py's FlatSGD twin, the first step's weights within Adam's own first
move, 2 lr, of the eager ones. Every test prints its figures before it asserts (pytest -s).

Worst observed on an MI355X over the ten stage cases: 1.23 u (|m| + S), 4.00 u (b2 v + (1 - b2) S^2), 4.60 u (|p| + |delta_k|),
informative fraction 0.907 .. 1.000; fused and literal paths both 4.8e-08 / 1.0e-07 / 1.5e-07 of max |p| off float64 over
the three steps."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import adam_ref as R
import fine_tuning_common as ft

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARAM_BAR = 1e-6          # of max |p|, max-norm (tests/test_fine_tuning_gpu.py)
N_STAGES = 100032         # 1563 blocks of 64
KEYS = ["model.model.conv_last.weight", "model.model.conv_last.bias"]
POISON = 1e3              # coefficient of the blocks outside the stepped range: a table indexed relative to `lo` reads it


@pytest.fixture(scope="module")
def N():
    import _native
    return _native


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).cuda()                  # a copy: adam_ref's arrays are read-only
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def anchors_and_coefficients(p, seed=77):
    """a = float32(p (1 + 0.25 N(0, 1))) and one coefficient per 64-element block, log-uniform in [1e-6, 1e-1]."""
    rng = np.random.default_rng(seed)
    a = (p.astype(np.float64) * (1.0 + 0.25 * rng.standard_normal(p.size))).astype(np.float32)
    c = np.exp(rng.uniform(np.log(1e-6), np.log(1e-1), p.size // 64)).astype(np.float32)
    return a, c


def restated_gradient(p, g, a, c_blocks, grad_scale):
    """g' in numpy float32, operation by operation in the documented order: g' = gs g; d = p - a; g' = g' + (2 c) d."""
    f = np.float32
    c = np.repeat(c_blocks.astype(f), 64)
    gp = f(grad_scale) * g.astype(f)
    d = p.astype(f) - a.astype(f)
    gp = gp + (f(2) * c) * d
    assert gp.dtype == f
    return gp


def penalties(p, a, c_blocks):
    """(float32 restatement summed by numpy in float32, float64 sum) of c d^2."""
    f = np.float32
    c = np.repeat(c_blocks.astype(f), 64)
    d = p.astype(f) - a.astype(f)
    ref32 = float(np.sum((c * d) * d, dtype=f))
    d64 = p.astype(np.float64) - a.astype(np.float64)
    return ref32, float(np.sum(c.astype(np.float64) * d64 * d64))


class Buffers:
    """Bucket-long device buffers (p, g, m, v, anchor, bf16 copy) filled with a recognisable pattern, the case's values at
    [lo, lo + n); a coefficient table with POISON on every block outside the range; copies of all of it as it was."""

    def __init__(self, arrays, a, c_blocks, lo, total):
        n = arrays[0].size
        assert lo % 64 == 0 and total % 64 == 0 and lo + n <= total and n % 64 == 0
        self.lo, self.hi, self.total = lo, lo + n, total
        rng = np.random.default_rng(7)
        self.f32 = []
        for values in (*arrays, a):
            back = rng.uniform(1.0, 2.0, total).astype(np.float32)
            back[lo:lo + n] = values
            self.f32.append(dev(back))
        self.p, self.g, self.m, self.v, self.a = self.f32
        self.p16 = dev(rng.uniform(1.0, 2.0, total).astype(np.float32), torch.bfloat16)
        table = np.full(total // 64, POISON, np.float32)
        table[lo // 64:(lo + n) // 64] = c_blocks
        self.coef = dev(table)
        self.before = [t.clone() for t in (*self.f32, self.p16)]
        self.penalty = torch.full((), -1.0, device="cuda")
        assert all(t.data_ptr() % 16 == 0 for t in (*self.f32, self.p16))

    def step(self, N, hyper, grad_scale=1.0, anchor=True, cap=0, shadow=True):
        count = N.lib().sei_adam_anchor_partials(self.lo, self.hi, cap)
        assert count == N.lib().sei_sgd_partials(self.lo, self.hi, cap) > 0
        parts = torch.full((count + 2,), -7.0, dtype=torch.float64, device="cuda")
        N.call("sei_adam_anchor_fused", self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
               self.a.data_ptr() if anchor else None, self.coef.data_ptr() if anchor else None, self.lo, self.hi,
               *hyper[:5], hyper.step, grad_scale, self.p16.data_ptr() if shadow else None,
               parts.data_ptr() if anchor else None, cap)
        if anchor:
            N.call("sei_sgd_penalty_finish", parts.data_ptr(), count, self.penalty.data_ptr())
        torch.cuda.synchronize()
        assert float(parts[count]) == -7.0 and float(parts[count + 1]) == -7.0     # no partial past the count
        return self

    def inside(self):
        return tuple(t[self.lo:self.hi] for t in (self.p, self.m, self.v, self.p16))

    def check_outside(self, what):
        now = (*self.f32, self.p16)
        for k, (t, t0) in enumerate(zip(now, self.before)):
            assert same_bits(t[:self.lo], t0[:self.lo]) and same_bits(t[self.hi:], t0[self.hi:]), \
                f"{what}: buffer {k} changed outside [{self.lo}, {self.hi})"
        assert same_bits(self.g, self.before[1]) and same_bits(self.a, self.before[4]), f"{what}: an input was written"


def reference_adam(N, arrays, hyper, grad_scale):
    """sei_adam_fused on fresh aligned copies: (p, m, v, bf16 copy) after the step."""
    p, g, m, v = (dev(x) for x in arrays)
    p16 = torch.zeros(p.numel(), device="cuda", dtype=torch.bfloat16)
    N.call("sei_adam_fused", p.data_ptr(), g.data_ptr(), 0, m.data_ptr(), v.data_ptr(), p.numel(), *hyper[:5], hyper.step,
           grad_scale, p16.data_ptr())
    torch.cuda.synchronize()
    return p, m, v, p16


@pytest.fixture(scope="module")
def stage_inputs():
    """Per first_step flag: (p, g, m, v), anchors and coefficients of the 100032-element range, built once."""
    out = {}
    for first in (False, True):
        arrays = R.state(N_STAGES, first_step=first)
        out[first] = (arrays,) + anchors_and_coefficients(arrays[0])
    return out


# ------------------------------------------------------------------ the kernel against float64
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("hyper", R.HYPER_SETS, ids=lambda h: f"step{h.step}")
def test_stages_against_float64(N, stage_inputs, hyper, grad_scale):
    """The range starts at block 3 of a longer bucket; (p', m', v') against the float64 model of one Adam step on g'."""
    arrays, a, c = stage_inputs[hyper.step == 1]
    p, g, m, v = arrays
    gp = restated_gradient(p, g, a, c, grad_scale)
    share = R.informative_fraction(p, gp, m, v, hyper)
    visible = float(np.mean(np.abs(gp - np.float32(grad_scale) * g) > 1e-3 * np.abs(np.float32(grad_scale) * g)))
    b = Buffers(arrays, a, c, lo=192, total=192 + N_STAGES + 64).step(N, hyper, grad_scale)
    pk, mk, vk, p16 = b.inside()
    worst = R.stage_errors(p, gp, m, v, host(pk), host(mk), host(vk), hyper)[0]
    ref32, ref64 = penalties(p, a, c)
    got = float(b.penalty)
    bar = ft.penalty_bar(ref32, ref64)
    print(f"ADAM-ANCHOR-WORST {hyper} gs={grad_scale} m={worst.m:.3f} v={worst.v:.3f} p={worst.p:.3f}; informative "
          f"{share:.3f}; penalty term visible on {visible:.3f}; penalty {got:.9e} vs float64 {ref64:.9e} (error "
          f"{abs(got - ref64):.2e}, float32 restatement error {abs(ref32 - ref64):.2e}, bar {bar:.2e})")
    assert share >= R.MIN_INFORMATIVE
    R.check_stages(p, gp, m, v, host(pk), host(mk), host(vk), hyper, grad_scale=1.0, what="sei_adam_anchor_fused")
    assert same_bits(p16, pk.bfloat16())
    assert b.penalty.dtype == torch.float32 and abs(got - ref64) <= bar, (got, ref64, bar)
    b.check_outside(f"{hyper} gs={grad_scale}")


# ------------------------------------------------------------------ bit identities
def test_without_an_anchor_it_is_sei_adam_fused(N, stage_inputs):
    hyper, grad_scale = R.HYPER_SETS[1], 0.125
    arrays, a, c = stage_inputs[False]
    want = reference_adam(N, arrays, hyper, grad_scale)
    b = Buffers(arrays, a, c, lo=192, total=192 + N_STAGES + 64).step(N, hyper, grad_scale, anchor=False)
    for name, got, ref in zip(("p", "exp_avg", "exp_avg_sq", "bf16 copy"), b.inside(), want):
        assert same_bits(got, ref), name
    assert float(b.penalty) == -1.0                               # nothing wrote a penalty
    b.check_outside("no anchor")
    # and without the bf16 copy: the same float32 bits, the copy untouched
    b2 = Buffers(arrays, a, c, lo=192, total=192 + N_STAGES + 64).step(N, hyper, grad_scale, anchor=False, shadow=False)
    for got, ref in zip(b2.inside()[:3], want[:3]):
        assert same_bits(got, ref)
    assert same_bits(b2.p16, b2.before[5])


@pytest.mark.parametrize("hyper", [R.HYPER_SETS[0], R.HYPER_SETS[1]], ids=lambda h: f"step{h.step}")
def test_at_the_anchor_it_is_sei_adam_fused_and_the_penalty_is_zero(N, stage_inputs, hyper):
    arrays, _, c = stage_inputs[hyper.step == 1]
    want = reference_adam(N, arrays, hyper, 1.0)
    b = Buffers(arrays, arrays[0], c, lo=192, total=192 + N_STAGES + 64).step(N, hyper, 1.0)
    for name, got, ref in zip(("p", "exp_avg", "exp_avg_sq", "bf16 copy"), b.inside(), want):
        assert same_bits(got, ref), name
    assert float(b.penalty) == 0.0


def _loop_case():
    arrays = R.state(9344, seed=2)
    return (arrays,) + anchors_and_coefficients(arrays[0], seed=78)


def test_capped_and_library_grids_agree(N):
    """9344 elements from lo = 64: the library's grid is 5 workgroups and one trip; capped at 2 workgroups it is two
    two-quad trips and a single-quad tail for 288 of the 512 threads. Same p, m, v and bf16 copy; the penalty's partial
    sums are grouped differently (2 against 5), so it agrees to double rounding only."""
    hyper = R.HYPER_SETS[1]
    arrays, a, c = _loop_case()
    assert N.lib().sei_adam_anchor_partials(64, 64 + 9344, 2) == 2 and N.lib().sei_adam_anchor_partials(64, 64 + 9344, 0) == 5
    runs = [Buffers(arrays, a, c, lo=64, total=9344 + 128).step(N, hyper, 1.0, cap=cap) for cap in (2, 0)]
    for name, x, y in zip(("p", "exp_avg", "exp_avg_sq", "bf16 copy"), runs[0].inside(), runs[1].inside()):
        assert same_bits(x, y), name
    gp = restated_gradient(arrays[0], arrays[1], a, c, 1.0)
    for r in runs:
        pk, mk, vk, _ = r.inside()
        R.check_stages(arrays[0], gp, arrays[2], arrays[3], host(pk), host(mk), host(vk), hyper, what="loop shapes")
        r.check_outside("loop shapes")
    ref32, ref64 = penalties(arrays[0], a, c)
    print(f"penalty capped {float(runs[0].penalty):.9e}, library grid {float(runs[1].penalty):.9e}, float64 {ref64:.9e}")
    for r in runs:
        assert abs(float(r.penalty) - ref64) <= ft.penalty_bar(ref32, ref64)


def test_two_runs_give_the_same_bits(N):
    hyper = R.HYPER_SETS[4]
    arrays, a, c = _loop_case()
    runs = [Buffers(arrays, a, c, lo=64, total=9344 + 128).step(N, hyper, 0.125) for _ in range(2)]
    for name, x, y in zip(("p", "exp_avg", "exp_avg_sq", "bf16 copy"), runs[0].inside(), runs[1].inside()):
        assert same_bits(x, y), name
    assert float(runs[0].penalty) > 0 and same_bits(runs[0].penalty, runs[1].penalty)


# ------------------------------------------------------------------ edges
@pytest.mark.parametrize("n,lo,total", [(64, 64, 192), (2048, 192, 192 + 2048 + 64), (2112, 192, 192 + 2112 + 64)])
def test_edges(N, n, lo, total):
    """One block (a quarter of a wave), one full workgroup trip, and one element block more (two workgroups): per-block
    coefficients read at the absolute block, sentinels on both sides of all four written streams, and padding elements
    (p = a = 0, g = m = v = 0) that stay exactly zero."""
    hyper = R.HYPER_SETS[1]                                     # weight decay 0.01: wd * 0 must still be 0
    p, g, m, v = (x.copy() for x in R.state(n, seed=8))
    a, c = anchors_and_coefficients(p, seed=79)
    pad = np.zeros(n, bool)
    pad[n - 29:] = True                                         # the tail of the last block, as models/_flat.py pads
    pad[5] = True
    for x in (p, g, m, v, a):
        x[pad] = 0
    assert len(set(c.tolist())) == n // 64
    assert N.lib().sei_adam_anchor_partials(lo, lo + n, 0) == (2 if n > 2048 else 1)
    b = Buffers((p, g, m, v), a, c, lo=lo, total=total).step(N, hyper, 1.0)
    pk, mk, vk, p16 = b.inside()
    gp = restated_gradient(p, g, a, c, 1.0)
    worst = R.check_stages(p, gp, m, v, host(pk), host(mk), host(vk), hyper, what=f"n={n}")
    ref32, ref64 = penalties(p, a, c)
    print(f"n={n} lo={lo}: m={worst.m:.3f} v={worst.v:.3f} p={worst.p:.3f}; penalty {float(b.penalty):.9e} vs {ref64:.9e}")
    b.check_outside(f"n={n}")
    padded = torch.from_numpy(pad).cuda()
    for name, t in zip(("p", "exp_avg", "exp_avg_sq", "bf16 copy"), (pk, mk, vk, p16)):
        assert not bits(t[padded]).any(), f"n={n}: {name} of a padding element is not +0"
    assert same_bits(p16, pk.bfloat16())
    assert abs(float(b.penalty) - ref64) <= ft.penalty_bar(ref32, ref64)


# ------------------------------------------------------------------ FlatAdam
def _fill(model, values=None, grads=None):
    with torch.no_grad():
        for name, p in model.named_parameters():
            if values is not None:
                p.copy_(torch.as_tensor(np.asarray(values[name])).to(p.device))
            if grads is not None:
                p._sei_grad_view.copy_(torch.as_tensor(np.asarray(grads[name])).to(p.device))


def _random_like(model, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return {n: scale * torch.randn(p.shape, generator=gen) for n, p in model.named_parameters()}


def test_flat_adam_construction_on_the_device():
    from optim import FlatAdam
    model = ft.Nested(seed=3).to("cuda")
    opt = FlatAdam(model, lr=1e-3, anchor=True)
    assert opt.last_penalty.is_cuda and opt.last_penalty.dim() == 0 and float(opt.last_penalty) == 0.0
    assert opt.anchor.is_cuda and opt.coef64.is_cuda and opt._ranges == [(0, model.get_backbone().flat_params.numel())]


def test_frozen_ranges():
    """only = the conv_last pair of a nested model, bf16 mode, non-zero gradients and moments everywhere: nothing outside
    the two ranges changes in the weights, both moments or the bf16 copy; inside, the step is the model's on the restated
    gradient and the copy is the rounded new weight; the penalty over the two ranges is the whole bucket's, which an
    lr = 0 whole-bucket FlatAdam reads."""
    from models import _ops
    from optim import FlatAdam
    lr, betas, eps, step = 1e-3, (0.9, 0.999), 1e-8, 2
    model = ft.Nested(seed=3).to("cuda")
    bb = model.get_backbone()
    bb.compute_dtype = "bf16"
    anchors = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    opt = FlatAdam(model, lr=lr, betas=betas, eps=eps, anchor=True, lambd=1, only=KEYS)
    whole = FlatAdam(model, lr=0.0, anchor=True, lambd=1)      # same anchor; lr = 0: reads the penalty, moves nothing
    current = dict(anchors)
    for k, v in _random_like(model, 44, 0.1).items():
        if k in KEYS:
            current[k] = anchors[k] + v
    grads = _random_like(model, 45)
    _fill(model, current, grads)
    assert all(bool((p._sei_grad_view != 0).all()) for p in model.parameters())
    st = opt.state[bb.flat_params]
    gen = torch.Generator().manual_seed(46)
    st["exp_avg"].copy_(0.01 * torch.randn(st["exp_avg"].shape, generator=gen))
    st["exp_avg_sq"].copy_(1e-4 * torch.rand(st["exp_avg_sq"].shape, generator=gen) + 1e-8)
    st["step"] = step - 1
    pad = ft.padding_mask(model).cuda()
    st["exp_avg"][pad] = 0                                    # the padding carries no state: it must stay exactly zero
    st["exp_avg_sq"][pad] = 0
    _ops.refresh_plain_shadow(bb)
    p_before, s_before = bb.flat_params.clone(), bb.flat_shadow.clone()
    m_before, v_before = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    whole.step()
    assert torch.equal(bb.flat_params.view(torch.int32), p_before.view(torch.int32))
    full_penalty = whole.last_penalty.clone()
    ranges = opt._ranges
    assert len(ranges) == 2 and all(lo % 64 == 0 and hi % 64 == 0 for lo, hi in ranges)
    opt.step()
    torch.cuda.synchronize()
    assert st["step"] == step
    inside = torch.zeros(bb.flat_params.numel(), dtype=torch.bool, device="cuda")
    for lo, hi in ranges:
        inside[lo:hi] = True
    for name, now, was in (("weights", bb.flat_params, p_before), ("exp_avg", st["exp_avg"], m_before),
                           ("exp_avg_sq", st["exp_avg_sq"], v_before), ("bf16 copy", bb.flat_shadow, s_before)):
        assert same_bits(now[~inside], was[~inside]), f"{name} changed outside the two ranges"
    for k in KEYS:
        assert not torch.equal(model.get_parameter(k).detach().cpu(), current[k])
    assert same_bits(bb.flat_shadow[inside], bb.flat_params[inside].to(torch.bfloat16))
    assert _ops.plain_shadow_is_current(bb)
    assert not bb.flat_params[pad].any() and not st["exp_avg"][pad].any() and not st["exp_avg_sq"][pad].any()
    # inside: the float64 model on the restated gradient (coefficients from the names alone)
    sel = host(inside)
    f = np.float32
    p0, a0 = host(p_before)[sel], ft.per_element(model, anchors, torch.float32).numpy()[sel]
    c0 = ft.coefficients(model).numpy().astype(f)[sel]
    gp = host(bb.flat_grads)[sel] + (f(2) * c0) * (p0 - a0)
    hyper = R.Hyper(lr, *betas, eps, 0.0, step)
    worst = R.check_stages(p0, gp, host(m_before)[sel], host(v_before)[sel], host(bb.flat_params)[sel],
                           host(st["exp_avg"])[sel], host(st["exp_avg_sq"])[sel], hyper, what="frozen ranges")
    d64 = ft.per_element(model, current) - ft.per_element(model, anchors)
    ref64 = float((ft.coefficients(model) * d64 * d64).sum())
    d32 = (p0 - a0).astype(f)
    ref32 = float(np.sum((c0 * d32) * d32, dtype=f))
    bar = ft.penalty_bar(ref32, ref64)
    print(f"frozen ranges: m={worst.m:.3f} v={worst.v:.3f} p={worst.p:.3f}; penalty over the two ranges "
          f"{float(opt.last_penalty):.9e}, over the whole bucket {float(full_penalty):.9e}, float64 {ref64:.9e} (bar {bar:.2e})")
    assert ref64 > 0 and abs(float(opt.last_penalty) - ref64) <= bar and abs(float(full_penalty) - ref64) <= bar
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
    """Three steps of FlatAdam(anchor=True, lambd=100) beside torch.optim.Adam on the same external gradients plus the
    autograd gradients of the torch WeightsDistanceLoss, both float32 on the GPU, both against the same three steps in
    float64 on the CPU: the fused path's error is at most twice the literal path's own at every step."""
    from losses.weights_distance_loss import WeightsDistanceLoss
    from optim import FlatAdam
    lambd, lr, b1, b2, eps = 100.0, 1e-3, 0.9, 0.999, 1e-8
    _, _, fused = _small_unet()
    _, _, literal = _small_unet()
    fb, lb = fused.get_backbone(), literal.get_backbone()
    assert torch.equal(fb.flat_params, lb.flat_params)
    opt = FlatAdam(fused, lr=lr, betas=(b1, b2), eps=eps, anchor=True, lambd=lambd)
    wd = WeightsDistanceLoss(pretrained_model=literal, lambd=lambd, device="cuda")
    adam = torch.optim.Adam(literal.parameters(), lr=lr, betas=(b1, b2), eps=eps)
    pad = ft.padding_mask(fused)
    c64 = ft.coefficients(fused, lambd)
    p64 = fb.flat_params.detach().cpu().double()
    a64 = p64.clone()
    m64, v64 = torch.zeros_like(p64), torch.zeros_like(p64)
    figures = []
    for step in range(3):
        g = torch.randn(fb.flat_grads.shape, generator=torch.Generator().manual_seed(50 + step))
        g[pad] = 0
        fb.flat_grads.copy_(g.cuda())
        lb.flat_grads.copy_(g.cuda())
        # float64
        d64 = p64 - a64
        pen64 = float((c64 * d64 * d64).sum())
        g64 = g.double() + 2 * c64 * d64
        m64 = m64 + (g64 - m64) * (1 - b1)
        v64 = b2 * v64 + (1 - b2) * g64 * g64
        t = step + 1
        p64 = p64 - (lr / (1 - b1 ** t)) * (m64 / (v64.sqrt() / np.sqrt(1 - b2 ** t) + eps))
        # literal float32
        value = wd(literal)
        penalty_grads = torch.autograd.grad(value, list(literal.parameters()))
        for prm, pg in zip(literal.parameters(), penalty_grads):
            prm.grad = prm._sei_grad_view + pg
        adam.step()
        opt.step()
        torch.cuda.synchronize()
        scale = float(p64.abs().max())
        err_fused = float((fb.flat_params.detach().cpu().double() - p64).abs().max()) / scale
        err_literal = float((lb.flat_params.detach().cpu().double() - p64).abs().max()) / scale
        figures.append((err_fused, err_literal, float(opt.last_penalty), float(value.detach()), pen64))
        print(f"step {step}: against float64, fused {err_fused:.3e}, literal {err_literal:.3e} of max |p| = {scale:.3f}; "
              f"penalty fused {float(opt.last_penalty):.6e}, literal {float(value.detach()):.6e}, float64 {pen64:.6e}")
    for step, (err_fused, err_literal, pen, value, pen64) in enumerate(figures):
        assert err_fused <= 2 * err_literal, (step, err_fused, err_literal)
        if step == 0:
            assert pen == 0.0 == value
        else:
            assert pen > 0 and value > 0
    assert not fb.flat_params[pad.cuda()].any()


def test_captured_step_with_flat_adam_matches_eager():
    """GraphedLossStep + FlatAdam(anchor=True).step() against zero_grad + loss + backward + the same step with the step's
    draws injected, two steps. First step, same weights on both sides: loss to 1e-6 relative, the gradient bucket to 1e-5
    of its largest entry (the float atomics' arrival order); Adam's first step moves a weight by at most lr on either
    side, so the weights agree within 2 lr (1 + 1e-6) plus the step's rounding. Second step: loss and gradient norm to
    2e-3. The kernel's arithmetic is pinned by the tests above, not here."""
    from graphs import GraphedLossStep
    from losses import get_loss
    from losses.sure import embed_probe
    from optim import FlatAdam
    B, lr = 4, 1e-3
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
        opt = FlatAdam(model, lr=lr, anchor=True)
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
        pdiff = float((pe - pg).abs().max())
        print(f"step {step}: loss {lg:.8e} (graph) vs {le:.8e} (eager); gradients {gerr:.1e}; weights differ by {pdiff:.2e} "
              f"(lr {lr:.0e}, max |p| {float(pe.abs().max()):.3f}); penalty {ng:.6e} vs {ne:.6e}")
        if step == 0:
            assert abs(le - lg) <= 1e-6 * abs(le), (le, lg)
            assert gerr < 1e-5, gerr
            assert pdiff <= 2 * lr * (1 + 1e-6) + PARAM_BAR * float(pe.abs().max())
        else:
            assert abs(le - lg) <= 2e-3 * abs(le), (le, lg)
            assert abs(float(ge.norm()) - float(gg.norm())) <= 2e-3 * float(ge.norm())
    assert runs["graph"][0][3] == 0.0 == runs["eager"][0][3] and runs["graph"][1][3] > 0 and runs["eager"][1][3] > 0
    assert not torch.equal(runs["graph"][0][2], runs["graph"][1][2])


def test_train_script_fine_tuning_with_adam(tmp_path):
    """train.py --fine_tuning --optimizer Adam --weights_distance_loss: the first step replays a hipGraph (FlatAdam with
    the penalty folded in), the losses are finite, the weights move and the checkpoint holds torch.optim.Adam's state
    over every parameter; with --no-fused_optimizer the same command runs the literal sequence eagerly."""
    from PIL import Image
    folder = tmp_path / "measurements"
    folder.mkdir()
    rng = np.random.default_rng(0)
    for k in range(3):
        Image.fromarray(rng.integers(0, 256, size=(64, 64, 3), dtype=np.uint8)).save(folder / f"y{k}.png")
    _, _, model = _small_unet()
    shapes = [tuple(p.shape) for p in model.parameters()]
    start = {k: v.detach().cpu().clone() for k, v in model.get_weights().items()}
    torch.save(start, tmp_path / "start.pt")
    out = tmp_path / "run"
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--device", "cuda", "--task", "deblurring", "--kernel",
           "Gaussian_R2", "--ProposedModel__architecture", "Convolutional", "--ConvolutionalModel__hidden_channels",
           "8", "--ConvolutionalModel__scales", "3", "--dataset", str(folder), "--PrepareTrainingPairs__crop_size", "64",
           "--batch_size", "2", "--epochs", "2", "--method", "proposed", "--fine_tuning", "--weights_distance_loss",
           "--optimizer", "Adam", "--lr", "1e-3",
           "--lr_scheduler_kind", "multi_step_decay",
           "--weights", str(tmp_path / "start.pt"), "--out_dir", str(out)]
    env = dict(os.environ, SEI_TRACE_STEP_KIND="1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "step kind: hipGraph replay" in r.stdout, r.stdout
    assert "Selected learning rate: 1.000000e-03" in r.stdout and "Selected optimizer: Adam" in r.stdout, r.stdout
    rows = open(out / "training.csv").read().strip().splitlines()
    assert rows[0] == "Epoch,Training Loss" and len(rows) == 3
    assert all(np.isfinite(float(r_.split(",")[1])) for r_ in rows[1:])
    w = torch.load(out / "weights.pt", map_location="cpu")
    assert set(w) == set(start) and any(not torch.equal(w[k], start[k]) for k in start)
    state = torch.load(out / "checkpoints" / "ckp_2.pt", map_location="cpu")["optimizer"]["state"]
    steps = 2 * 2                                             # two epochs of three files in batches of two
    assert sorted(state) == list(range(len(shapes)))
    for i, shape in enumerate(shapes):
        assert tuple(state[i]["exp_avg"].shape) == shape == tuple(state[i]["exp_avg_sq"].shape)
        assert float(state[i]["step"]) == steps
    assert any(bool(state[i]["exp_avg"].any()) for i in state)
    r = subprocess.run(cmd[:-1] + [str(tmp_path / "run2"), "--no-fused_optimizer"], capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "step kind: eager" in r.stdout and "Selected optimizer: Adam" in r.stdout, r.stdout
