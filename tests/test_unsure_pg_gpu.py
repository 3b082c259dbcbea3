"""Poisson-Gaussian UNSURE on the GPU: sei_sure_loss_unsure_pg and sei_axpy_hetero_dev through the C ABI,
SurePoissonGaussianLoss, a replayed step against an eager one, train.py --unsure_noise_model poisson_gaussian end to end, and
the statistics of physics._base.PoissonGaussianNoise.

Bars, by tests/test_unsure_gpu.py's rules. The three sums, the loss value, g1 and g2 of the kernel grid: max(5e-6, 3 * ref32) of
float64 (streaming_ref.bar), ref32 being the deviation of tests/unsure_pg_ref.py's float32 chain from its float64 one; the sums
relative to the float64 sum of their absolute terms (D1 as D0), the loss to |mse| + 2 (|eta| mean|d0 terms| + |gamma|
mean|d1 terms|), the gradients to their largest element. The state update: unsure_ref.ascent in float64 per multiplier on the
kernel's OWN sum, m' and the value within unsure_ref.state_bar (8 * 2^-24 of max(|value|, |alpha m'|, |m'|): at most four
float32 roundings each). sei_axpy_hetero_dev: 3 ulp of the float64 result (test_axpy_hetero_dev derives it). The module's
trajectory: the per-step bars above, times K for the state after K steps. With gamma = 0 against sei_sure_loss_unsure, and
replay against eager: equality of bits.

Measured on one MI355X (largest over the cases of a family):
    family                                  ref32     bar        HIP deviation
    D0 sum  (of sum |terms|)                6.9e-8    5.0e-6     8.0e-8
    D1 sum  (of sum |terms|)                6.5e-8    5.0e-6     9.4e-8
    mse sum                                 1.1e-7    5.0e-6     4.8e-8
    loss value (of its scale)               6.0e-8    5.0e-6     6.0e-8
    g1                                      1.2e-7    5.0e-6     1.2e-7
    g2                                      1.0e-7    5.0e-6     1.0e-7
    m' after one update (of the bar)        --        1.0        0.021 (eta), 0.050 (gamma)
    value after one update (of the bar)     --        1.0        0.082 (eta), 0.057 (gamma)
    sei_axpy_hetero_dev (ulp of result)     --        3.0        0.883
    trajectory, 6 steps: eta / gamma        --        1.0        0.0035 / 0.0149
    trajectory, 6 steps: m_eta / m_gamma    --        1.0        0.0008 / 0.0015
    trajectory, per step: loss              3.4e-8    5.0e-6     2.2e-8
    trajectory, per step: y1.grad           1.2e-7    5.0e-6     1.4e-7
    trajectory, per step: y2.grad           1.1e-7    5.0e-6     1.2e-7
(the kernel grid's nine runs; over every state update of the module, the largest is 0.072 for m' and 0.082 for a value.)
PoissonGaussianNoise at the test's seed: mean -0.39 and variance -0.92 standard errors from their expectations, correlation
with the next normal draw +0.0007 (standard error 0.0020).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import loss_reduction_ref as L
import streaming_ref as R
import unsure_pg_ref as P
import unsure_ref as U

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
BLOCKS = 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ETA, GAMMA = float(L.f32(0.01)), float(L.f32(0.03))

# the seven loss_reduction_ref.SURE_CASES entries tests/test_unsure_gpu.py runs, as (planes, H, W, margin_div, margin_mse)
GRID = [(1, 1, 1, 0, 0), (1, 5, 9, 1, 2), (2, 7, 7, 3, 3), (5, 3, 17, 0, 1), (3, 48, 48, 6, 6), (4, 256, 256, 0, 0),
        (7, 200, 190, 6, 3)]
CASES = [next(c for c in L.SURE_CASES if c[:5] == g) for g in GRID]


def native():
    import _native
    assert _native.SEI_REDUCE_BLOCKS == BLOCKS
    return _native


def ids(case):
    return "x".join(str(int(v)) for v in case) if isinstance(case, tuple) else None


class Out:
    """A Guarded output whose first element lies `lead` floats behind the front margin (tests/test_unsure_gpu.py)."""

    def __init__(self, shape, lead=0):
        n = int(torch.Size(shape if isinstance(shape, (tuple, list)) else (shape,)).numel())
        self.guard, self.lead = R.Guarded(n + lead), lead
        self.view = self.guard.view[lead:].view(shape)

    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        return self.guard.intact() and bool((self.guard.view[:self.lead] == R.SENTINEL).all())


def counts(case):
    planes, H, W, md, mm, _ = case
    return planes * (H - 2 * md) * (W - 2 * md), planes * (H - 2 * mm) * (W - 2 * mm)


def pg_state(eta=ETA, gamma=GAMMA, m_eta=0.0, m_gamma=0.0, k=0.0, spare=(0.0, 0.0, 0.0)):
    return [eta, m_eta, k, spare[0], gamma, m_gamma, spare[1], spare[2]]


def operands(case, lead, joint):
    """The inputs of one call on the device, NaN-framed -> (y, b, y1 pointer, y2 pointer, gradient outputs, g1 view, g2 view)."""
    planes, H, W = case[:3]
    y, y1, y2, b = L.sure_inputs(*case)
    put = (lambda t: R.nan_framed(t, lead)) if lead else R.nan_tailed
    yd, bd = put(y), put(b)
    if joint:
        y12 = put(torch.stack([y1, y2]))
        g12 = Out((2, planes, H, W), lead)
        keep, p1, p2, outs, v1, v2 = y12, y12[0].data_ptr(), y12[1].data_ptr(), [g12], g12.view[0], g12.view[1]
        assert p2 - p1 == 4 * y.numel() and v2.data_ptr() - v1.data_ptr() == 4 * y.numel()
    else:
        y1d, y2d, g1, g2 = put(y1), put(y2), Out((planes, H, W), lead), Out((planes, H, W), lead)
        keep, p1, p2, outs, v1, v2 = (y1d, y2d), y1d.data_ptr(), y2d.data_ptr(), [g1, g2], g1.view, g2.view
    assert not lead or all(p % 16 == 4 * lead for p in (yd.data_ptr(), bd.data_ptr(), p1, v1.data_ptr()))
    return (y, b, keep), yd, bd, p1, p2, outs, v1, v2


def run_pg(case, state, alpha_eta=1e-2, alpha_gamma=2e-2, mu=0.9, update=1, tau=L.TAU, joint=False, lead=0):
    """One sei_sure_loss_unsure_pg call on fresh buffers -> (out4, g1, g2, state after) on the CPU, the margins checked."""
    N = native()
    planes, H, W, md, mm, _ = case
    n_div, n_mse = counts(case)
    (y, b, _keep), yd, bd, p1, p2, outs, v1, v2 = operands(case, lead, joint)
    out, work, st = Out(4, lead), Out(3 * BLOCKS, lead), R.Guarded(8)
    st.view.copy_(torch.tensor(state, dtype=F32))
    assert st.ptr() % 16 == 0
    N.call("sei_sure_loss_unsure_pg", yd.data_ptr(), p1, p2, bd.data_ptr(), planes, H, W, md, mm, tau, 1.0 / n_mse,
           1.0 / n_div, alpha_eta, alpha_gamma, mu, update, st.ptr(), out.ptr(), v1.data_ptr(), v2.data_ptr(), work.ptr())
    torch.cuda.synchronize()
    assert out.intact() and work.intact() and st.intact() and all(g.intact() for g in outs), case
    assert R.same_bits(yd, y) and R.same_bits(bd, b)
    return out.view.cpu(), v1.cpu(), v2.cpu(), st.view.cpu()


def run_gaussian(case, state, alpha=1e-2, mu=0.9, update=1, tau=L.TAU):
    """The same call through sei_sure_loss_unsure with the four-float state -> (out3, g1, g2, state after)."""
    N = native()
    planes, H, W, md, mm, _ = case
    n_div, n_mse = counts(case)
    (y, b, _keep), yd, bd, p1, p2, outs, v1, v2 = operands(case, 0, False)
    out, work, st = Out(3), Out(2 * BLOCKS), R.Guarded(4)
    st.view.copy_(torch.tensor(state, dtype=F32))
    N.call("sei_sure_loss_unsure", yd.data_ptr(), p1, p2, bd.data_ptr(), planes, H, W, md, mm, tau, 1.0 / n_mse,
           1.0 / n_div, alpha, mu, update, st.ptr(), out.ptr(), v1.data_ptr(), v2.data_ptr(), work.ptr())
    torch.cuda.synchronize()
    assert out.intact() and work.intact() and st.intact() and all(g.intact() for g in outs), case
    return out.view.cpu(), v1.cpu(), v2.cpu(), st.view.cpu()


@functools.lru_cache(maxsize=None)
def references(case, eta, gamma, tau=L.TAU):
    """(float64, float32) restatements of one case: computed once, shared, never written to."""
    md, mm = case[3:5]
    inp = L.sure_inputs(*case)
    return tuple(P.pg_loss_and_grads(*inp, md, mm, tau, eta, gamma, dt) for dt in (F64, F32))


def hold_terms(label, case, got, eta, gamma, tau=L.TAU):
    """The three sums (the restatement's means times the counts), the loss and both gradients under streaming_ref's bars."""
    r64, r32 = references(case, eta, gamma, tau)
    n_div, n_mse = counts(case)
    out, g1, g2 = got[:3]
    for name, slot, key in (("D0", 0, "d0"), ("D1", 1, "d1")):
        R.hold32_on(f"{label} {name} sum", out[slot], r64[key] * n_div, r32[key].double() * n_div,
                    r64["abs_" + key] * n_div)
    R.hold32_on(label + " mse sum", out[2], r64["mse"] * n_mse, r32["mse"].double() * n_mse, r64["mse"] * n_mse)
    scale = float(r64["mse"]) + 2 * (abs(eta) * float(r64["abs_d0"]) + abs(gamma) * float(r64["abs_d1"]))
    R.hold32_on(label + " loss", out[3], r64["loss"], r32["loss"], scale)
    R.hold32(label + " g1", g1, r64["g1"], r32["g1"])
    if float(r64["g2"].abs().max()) > 0:
        R.hold32(label + " g2", g2, r64["g2"], r32["g2"])
    assert bool((g2[r64["g2"] == 0] == 0).all()), label + ": g2 is zero outside the divergence interior"


def hold_state(label, case, state, after, out, alpha_eta, alpha_gamma, mu):
    """Per multiplier: m' and the value against unsure_ref.ascent in float64 on the kernel's own sum and the float32-rounded
    arguments, within unsure_ref.state_bar; k' = k + 1 once; the three spare slots bit for bit. -> {name: (value64, m64)}."""
    before = torch.tensor(state, dtype=F32)
    inv_n_div, k = U.rounded(1.0 / counts(case)[0]), int(before[2])
    res = {}
    for name, slot, total, alpha in (("eta", 0, out[0], alpha_eta), ("gamma", 4, out[1], alpha_gamma)):
        v, m, alpha = float(before[slot]), float(before[slot + 1]), U.rounded(alpha)
        v64, m64, k64 = U.ascent(v, m, k, float(total) * inv_n_div, alpha, U.rounded(mu))
        bar = U.state_bar(v, m64, alpha)
        dev_m, dev_v = abs(float(after[slot + 1]) - m64), abs(float(after[slot]) - v64)
        print(f"{label} {name}: m' {float(after[slot + 1])!r} (float64 {m64!r}, apart {dev_m:.2e}), value "
              f"{float(after[slot])!r} (float64 {v64!r}, apart {dev_v:.2e}), bar {bar:.2e}: {dev_m / bar:.3f} and "
              f"{dev_v / bar:.3f} of it")
        assert dev_m <= bar and dev_v <= bar, (label, name)
        assert float(after[2]) == k64
        res[name] = (v64, m64)
    spare = [3, 6, 7]
    assert R.same_bits(after[spare], before[spare]), label
    return res


# ------------------------------------------------------------------------------------------------ 1. kernel against the restatement
GRID_RUNS = [(c, {}) for c in CASES] + [(L.SURE_JOINT, dict(joint=True)), (L.SURE_OFFSET, dict(lead=1))]


@pytest.mark.parametrize("case,kw", GRID_RUNS, ids=[ids(c) + "".join("-" + k for k in kw) for c, kw in GRID_RUNS])
def test_kernel_grid(case, kw):
    """Sums, loss and both gradients with eta = 0.01 and gamma = 0.03 in device memory, the first update riding along (the
    gradients carry the multipliers as they stood before it); called again on the same state, the same bits everywhere.
    SURE_JOINT runs in the joint 2B layout, SURE_OFFSET 4 bytes off the 16-byte grid."""
    state = pg_state()
    got = run_pg(case, state, **kw)
    hold_terms(f"pg {ids(case)}", case, got, ETA, GAMMA)
    hold_state(f"pg {ids(case)}", case, state, got[3], got[0], 1e-2, 2e-2, 0.9)
    again = run_pg(case, state, **kw)
    assert all(R.same_bits(a, b) for a, b in zip(got, again))


STATE_CASE = next(c for c in L.SURE_CASES if c[:5] == (3, 48, 48, 6, 6))


@pytest.mark.parametrize("label,state,alphas,mu", [
    ("first call, stale directions ignored", pg_state(m_eta=3.0, m_gamma=-2.0), (1e-2, 2e-2), 0.9),
    ("later call", pg_state(0.0123, 0.021, 0.37, -0.11, 4.0), (1e-2, 2e-2), 0.9),
    ("later call, the default steps", pg_state(0.0123, 0.021, -0.05, 0.2, 7.0), (1e-4, 1e-4), 0.9),
    ("momentum 0", pg_state(0.0123, 0.021, 0.37, -0.11, 4.0), (1e-2, 5e-3), 0.0),
    ("the spare slots are left alone", pg_state(0.0123, 0.021, 0.37, -0.11, 2.0, spare=(42.0, -1.5, 7.0)), (1e-2, 2e-2), 0.5)])
def test_state_update(label, state, alphas, mu):
    got = run_pg(STATE_CASE, state, alpha_eta=alphas[0], alpha_gamma=alphas[1], mu=mu)
    hold_state(label, STATE_CASE, state, got[3], got[0], alphas[0], alphas[1], mu)
    if state[2] == 0.0 or mu == 0.0:
        inv = L.f32(1.0 / counts(STATE_CASE)[0])
        assert float(got[3][1]) == float(2 * (got[0][0] * inv)) and float(got[3][5]) == float(2 * (got[0][1] * inv)), \
            "m' = g exactly: one rounding, the kernel's own"
    hold_terms(label, STATE_CASE, got, float(L.f32(state[0])), float(L.f32(state[4])))


# ------------------------------------------------------------------------------------------------ 2. gamma = 0: the Gaussian kernel
@pytest.mark.parametrize("case", [CASES[4], CASES[5]], ids=ids)
@pytest.mark.parametrize("k,m_eta", [(0.0, 0.0), (4.0, 0.37)])
def test_gamma_zero_is_sei_sure_loss_unsure_bit_for_bit(case, k, m_eta):
    """gamma = 0 and step_gamma = 0: D0, the mse sum, the loss, g1, g2 and state[0..2] are sei_sure_loss_unsure's bits (a
    margin of 6 and none); D1 is finite, so gamma stays +0 whatever direction its slot carried."""
    state = pg_state(0.0123, 0.0, m_eta, 0.5, k)
    got = run_pg(case, state, alpha_eta=1e-2, alpha_gamma=0.0)
    ref = run_gaussian(case, state[:4], alpha=1e-2)
    assert R.same_bits(got[0][[0, 2, 3]], ref[0])
    assert R.same_bits(got[1], ref[1]) and R.same_bits(got[2], ref[2])
    assert R.same_bits(got[3][:3], ref[3][:3])
    assert bool(torch.isfinite(got[0][1])) and R.same_bits(got[3][4:5], torch.zeros(1))
    assert float(got[3][2]) == k + 1


# ------------------------------------------------------------------------------------------------ 3. determinism and flags
@pytest.mark.parametrize("case", [CASES[1], CASES[4], CASES[6]], ids=ids)
def test_update_0_leaves_the_state_bitwise_and_everything_else_the_same(case):
    state = pg_state(0.0123, 0.021, 0.37, -0.11, 4.0, spare=(-0.0, 3.0, -0.0))
    frozen, moved = run_pg(case, state, update=0), run_pg(case, state, update=1)
    assert R.same_bits(frozen[3], torch.tensor(state, dtype=F32))
    assert not R.same_bits(moved[3][:3], frozen[3][:3]) and not R.same_bits(moved[3][4:6], frozen[3][4:6])
    assert all(R.same_bits(a, b) for a, b in zip(frozen[:3], moved[:3]))


@pytest.mark.parametrize("which", ["eta", "gamma"])
def test_a_negative_sum_takes_its_multiplier_below_zero_unclamped(which):
    """The sign of tau flips both sums: with the one that makes D0 (or D1) negative, and a step that takes the multiplier
    about 0.1 below zero, the negative value is stored as it is, and the next call works with it as it stands."""
    case = CASES[1]
    key, slot = ("d0", 0) if which == "eta" else ("d1", 4)
    r64 = references(case, ETA, GAMMA)[0]
    tau = L.TAU if float(r64[key]) < 0 else -L.TAU
    d = -abs(float(r64[key]))
    assert abs(d) > 1e-3 * float(r64["abs_" + key])                 # a sum well clear of its rounding
    start = (ETA, GAMMA)[slot // 4]
    alpha = (start + 0.1) / (2 * abs(d))
    alphas = (alpha, 1e-3) if which == "eta" else (1e-3, alpha)
    state = pg_state()
    got = run_pg(case, state, alpha_eta=alphas[0], alpha_gamma=alphas[1], tau=tau)
    assert float(got[0][slot // 4]) < 0
    res = hold_state(f"negative {key}", case, state, got[3], got[0], alphas[0], alphas[1], 0.9)
    assert res[which][0] < -0.05 and float(got[3][slot]) < -0.05
    hold_terms(f"negative {key}", case, got, ETA, GAMMA, tau)
    after = [float(v) for v in got[3]]
    nxt = run_pg(case, after, alpha_eta=1e-3, alpha_gamma=1e-3, tau=tau)
    hold_terms(f"negative {which}", case, nxt, after[0], after[4], tau)
    hold_state(f"negative {which}", case, after, nxt[3], nxt[0], 1e-3, 1e-3, 0.9)


def test_joint_layout_and_storage_offset():
    """y1 | y2 and g1 | g2 as the halves of one 2B-image tensor (ProposedLoss's fused pass), and every operand, output and
    the workspace 4 bytes off the 16-byte grid (the state keeps its own alignment): the plain aligned call's bits."""
    state = pg_state(0.0123, 0.021, 0.37, -0.11, 4.0)
    for case, kw in ((L.SURE_JOINT, dict(joint=True)), (L.SURE_OFFSET, dict(lead=1)), (L.SURE_JOINT, dict(joint=True, lead=1))):
        got, plain = run_pg(case, state, **kw), run_pg(case, state)
        assert all(R.same_bits(a, b) for a, b in zip(got, plain)), kw


def test_refusals_touch_nothing():
    """Each refusal returns 10001 (SEI_ERR_BAD_ARG) and neither out4 nor the state nor anything else is written."""
    N = native()
    fn = N.lib().sei_sure_loss_unsure_pg
    H, W = 8, 6
    t = R.nan_tailed(torch.rand((2, H, W)))
    out, g1, g2, work, st = R.Guarded(4), R.Guarded((2, H, W)), R.Guarded((2, H, W)), R.Guarded(3 * BLOCKS), R.Guarded(8)
    ok = dict(y=t.data_ptr(), y1=t.data_ptr(), y2=t.data_ptr(), b=t.data_ptr(), planes=2, H=H, W=W, md=2, mm=2, tau=0.01,
              c_mse=0.01, inv_n_div=0.02, step_eta=1e-2, step_gamma=1e-2, mu=0.9, update=1, state=st.ptr(), out4=out.ptr(),
              g1=g1.ptr(), g2=g2.ptr(), work=work.ptr(), stream=N.stream())
    bad = [dict(state=None), dict(state=st.ptr() + 4), dict(state=st.ptr() + 8), dict(mu=-0.1), dict(mu=1.0), dict(mu=1.5),
           dict(mu=float("nan")), dict(step_eta=float("inf")), dict(step_eta=float("-inf")), dict(step_eta=float("nan")),
           dict(step_gamma=float("inf")), dict(step_gamma=float("-inf")), dict(step_gamma=float("nan")), dict(update=2),
           # what sei_sure_loss refuses: an empty interior for either margin on either axis, tau == 0, planes == 0, a null
           dict(md=3, mm=0), dict(md=0, mm=3), dict(H=W, W=H, md=3, mm=0), dict(H=W, W=H, md=0, mm=3), dict(H=H, W=H, md=4, mm=4),
           dict(tau=0.0), dict(planes=0), dict(y=None), dict(b=None), dict(out4=None), dict(g2=None), dict(work=None)]
    for change in bad:
        assert fn(*dict(ok, **change).values()) == 10001, change
        torch.cuda.synchronize()
        for g in (out, g1, g2, work, st):
            assert g.intact() and bool((g.view == R.SENTINEL).all()), change
    st.view.copy_(torch.tensor(pg_state()))
    assert fn(*ok.values()) == 0                                        # the same buffers, inside every bound
    torch.cuda.synchronize()
    assert bool((g1.view != R.SENTINEL).all()) and bool((out.view != R.SENTINEL).all()) and float(st.view[2]) == 1.0
    assert all(g.intact() for g in (out, g1, g2, work, st))


# ------------------------------------------------------------------------------------------------ 4. sei_axpy_hetero_dev
AXPY_N = [1, 3, 255, 1025, L.CAP + 1]
AXPY_ETA, AXPY_GAMMA = float(L.f32(1e-3)), float(L.f32(2e-2))


@functools.lru_cache(maxsize=None)
def axpy_inputs(n):
    """a uniform in [1, 2] and b ~ N(0, 1) cut off at +-3."""
    gen = L._gen(n, 59)
    return 1 + torch.rand(n, generator=gen), torch.randn(n, generator=gen).clamp(-3, 3)


def run_axpy(name, a, b, level):
    """sei_axpy_hetero_dev on an eight-float state, or sei_axpy_sqrt_dev on one float."""
    N = native()
    ad, bd, ld, out = R.nan_tailed(a), R.nan_tailed(b), R.nan_tailed(torch.tensor(level, dtype=F32)), R.Guarded(a.numel())
    N.call(name, ad.data_ptr(), bd.data_ptr(), ld.data_ptr(), out.ptr(), a.numel())
    torch.cuda.synchronize()
    assert out.intact() and R.same_bits(ad, a) and R.same_bits(bd, b) and R.same_bits(ld, torch.tensor(level, dtype=F32))
    return out.view.cpu()


def ulps_apart(got, r64):
    """|got - r64| in units of the float32 spacing at |r64|, largest over the elements (tests/test_unsure_gpu.py)."""
    mag = r64.abs().float()
    ulp = (torch.nextafter(mag, torch.full_like(mag, float("inf"))) - mag).double()
    return float(((got.double() - r64).abs() / ulp).max())


@pytest.mark.parametrize("n", AXPY_N)
def test_axpy_hetero_dev(n):
    """a + sqrt(max(gamma a + eta, 0)) b against float64 to 3 ulp of the result, with a in [1, 2], |b| <= 3, eta = 1e-3 and
    gamma = 2e-2: s = sqrt(w) <= 0.203, so |s b| <= 0.61 <= 1.6 |out| (|out| >= 1 - 0.61). The kernel rounds three times: the
    fused multiply-add under the root (half an ulp of w, halved by the root: a quarter of an ulp of s), the root (at most
    1 ulp of s) and the final fused multiply-add (half an ulp of the result): (1.25 ulp of s) |b| is at most 1.25 * 1.6 = 2
    ulp of the result, plus half: 2.5. gamma = 0 returns sei_axpy_sqrt_dev's bits; a root's argument at or below zero
    everywhere returns `a` bit for bit."""
    a, b = axpy_inputs(n)
    w = (AXPY_GAMMA * a.double() + AXPY_ETA).clamp_min(0)
    r64 = a.double() + w.sqrt() * b.double()
    assert float((w.sqrt() * b.double()).abs().max()) <= 0.61 <= 1.6 * float(r64.abs().min())
    got = run_axpy("sei_axpy_hetero_dev", a, b, pg_state(AXPY_ETA, AXPY_GAMMA, 0.3, -0.2, 5.0, spare=(1.0, 2.0, 3.0)))
    apart = ulps_apart(got, r64)
    print(f"axpy_hetero_dev n={n}: {apart:.3f} ulp of the float64 result")
    assert apart <= 3.0
    for eta in (AXPY_ETA, float(L.f32(L.SIGMA ** 2))):
        assert R.same_bits(run_axpy("sei_axpy_hetero_dev", a, b, pg_state(eta, 0.0, 0.3, -0.2, 5.0)),
                           run_axpy("sei_axpy_sqrt_dev", a, b, [eta]))
    for eta, gamma in ((0.0, 0.0), (-0.05, 0.02), (-1.0, 0.5), (-1e-3, 0.0), (-float("inf"), 0.02)):
        assert R.same_bits(run_axpy("sei_axpy_hetero_dev", a, b, pg_state(eta, gamma)), a), (eta, gamma)


def test_axpy_hetero_dev_host_layer():
    """physics._ops.axpy_hetero_dev and GaussianNoise.forward(noise_state_pg=): the kernel's bits, an operand off the 16-byte
    grid staged in a fresh allocation, an operand that needs a gradient refused (the level depends on it)."""
    from physics._base import GaussianNoise, PoissonGaussianNoise
    from physics._ops import axpy_hetero_dev
    a, b = axpy_inputs(1025)
    state = torch.tensor(pg_state(AXPY_ETA, AXPY_GAMMA), dtype=F32, device="cuda")
    want = run_axpy("sei_axpy_hetero_dev", a, b, pg_state(AXPY_ETA, AXPY_GAMMA))
    assert R.same_bits(axpy_hetero_dev(a.cuda(), b.cuda(), state), want)
    assert R.same_bits(axpy_hetero_dev(R.nan_framed(a, 1), R.nan_framed(b, 3), state), want)
    assert R.same_bits(GaussianNoise(sigma=0.5)(a.cuda(), noise=b.cuda(), noise_state_pg=state), want)
    # a Poisson-Gaussian model handed unit normals scales them to its own variance sigma^2 + gain a
    own = PoissonGaussianNoise(sigma=AXPY_ETA ** 0.5, gain=AXPY_GAMMA)(a.cuda(), noise=b.cuda())
    sigma2 = float(L.f32((AXPY_ETA ** 0.5) ** 2))
    assert R.same_bits(own, run_axpy("sei_axpy_hetero_dev", a, b, pg_state(sigma2, AXPY_GAMMA)))
    with pytest.raises(NotImplementedError):
        axpy_hetero_dev(a.cuda().requires_grad_(True), b.cuda(), state)
    with pytest.raises(ValueError):
        axpy_hetero_dev(a.cuda(), b.cuda(), state[:4].clone())


# ------------------------------------------------------------------------------------------------ 5. module
TRAJ = dict(steps=6, margin=2, sigma=0.1, gain=0.03, alpha_eta=5e-3, alpha_gamma=2e-3, mu=0.9)


def make_term(**over):
    from losses.sure import SurePoissonGaussianLoss
    kw = dict(sigma=TRAJ["sigma"], gain=TRAJ["gain"], margin=TRAJ["margin"], cropped_div=True, step_size=TRAJ["alpha_eta"],
              gain_step_size=TRAJ["alpha_gamma"], momentum=TRAJ["mu"])
    kw.update(over)
    return SurePoissonGaussianLoss(**kw).to("cuda")


def module_call(term, step):
    y, y1, y2, b = (t.cuda() for t in U.trajectory_inputs(step))
    y1.requires_grad_(True)
    y2.requires_grad_(True)
    loss = term(y=y, x_net=None, physics=None, model=None, b=b, y1=y1, y2=y2)
    loss.backward()
    return loss.detach().cpu(), y1.grad.cpu(), y2.grad.cpu(), term.noise_state.cpu().clone()


def test_module_trajectory():
    """Six training-mode calls on y1 / y2 given as autograd leaves at (2, 3, 16, 16), margin 2, against the float64 torch
    restatement. Per step: loss, y1.grad and y2.grad under the bars of the kernel grid. State after K steps, per multiplier:
    K times the per-step bar, which adds the two bars a step is held to (tests/test_unsure_gpu.py's test_module_trajectory) --
    the update's own, unsure_ref.state_bar, and its divergence mean's, max(5e-6, 3 ref32) of the mean of its absolute terms,
    which enters m' through g = 2 d (a factor 2) and the value through alpha m' (a factor 2 alpha)."""
    K = TRAJ["steps"]
    args = (K, TRAJ["margin"], L.TAU, TRAJ["sigma"] ** 2, TRAJ["gain"], TRAJ["alpha_eta"], TRAJ["alpha_gamma"], TRAJ["mu"])
    r64, r32 = P.trajectory(*args, dtype=F64), P.trajectory(*args, dtype=F32)
    term = make_term()
    start = torch.tensor(pg_state(TRAJ["sigma"] ** 2, TRAJ["gain"]), dtype=F32)
    assert term.training and R.same_bits(term.noise_state.cpu(), start)
    before = {"eta": float(start[0]), "gamma": float(start[4])}
    worst = {}
    for i in range(K):
        loss, g1, g2, state = module_call(term, i)
        a, c = r64[i], r32[i]
        eta64 = U.rounded(TRAJ["sigma"] ** 2) if i == 0 else r64[i - 1]["eta"]
        gamma64 = U.rounded(TRAJ["gain"]) if i == 0 else r64[i - 1]["gamma"]
        scale = float(a["mse"]) + 2 * (abs(eta64) * float(a["abs_d0"]) + abs(gamma64) * float(a["abs_d1"]))
        R.hold32_on(f"step {i + 1} loss", loss, a["loss"], c["loss"], scale)
        R.hold32(f"step {i + 1} y1.grad", g1, a["g1"], c["g1"])
        R.hold32(f"step {i + 1} y2.grad", g2, a["g2"], c["g2"])
        for name, slot, key, alpha in (("eta", 0, "d0", TRAJ["alpha_eta"]), ("gamma", 4, "d1", TRAJ["alpha_gamma"])):
            alpha = U.rounded(alpha)
            abs_d = float(a["abs_" + key])
            ref32_d = abs(float(c[key]) - float(a[key])) / abs_d
            own = U.state_bar(before[name], a["m_" + name], alpha)
            step_bar = own + 2 * R.bar(ref32_d) * abs_d
            bar_m, bar_v = (i + 1) * step_bar, (i + 1) * (own + alpha * step_bar)
            dev_m, dev_v = abs(float(state[slot + 1]) - a["m_" + name]), abs(float(state[slot]) - a[name])
            print(f"step {i + 1} {name}: value {float(state[slot])!r} (float64 {a[name]!r}, apart {dev_v:.2e}, bar {bar_v:.2e}), "
                  f"m {float(state[slot + 1])!r} (float64 {a['m_' + name]!r}, apart {dev_m:.2e}, bar {bar_m:.2e})")
            assert dev_m <= bar_m and dev_v <= bar_v, (i, name)
            worst[name] = max(worst.get(name, 0.0), dev_v / bar_v)
            worst["m_" + name] = max(worst.get("m_" + name, 0.0), dev_m / bar_m)
            before[name] = float(state[slot])
        assert float(state[2]) == i + 1 == a["k"] and R.same_bits(state[[3, 6, 7]], torch.zeros(3))
    print("trajectory: largest deviations of the bars: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(worst.items())))
    assert float(term.noise_state[0]) != float(start[0]) and float(term.noise_state[4]) != float(start[4])
    assert term.estimated_sigma() == max(float(term.noise_state[0]), 0.0) ** 0.5
    assert term.estimated_gain() == float(term.noise_state[4])


def test_module_in_eval_mode_and_state_dict():
    term = make_term()
    for i in range(2):
        module_call(term, i)
    moved = term.noise_state.cpu().clone()
    assert float(moved[2]) == 2.0 and moved.numel() == 8
    address = term.noise_state.data_ptr()
    term.eval()
    loss_eval, g1_eval, _, state = module_call(term, 2)
    assert R.same_bits(state, moved), "eval: the state does not move"
    term.train()
    loss_train, g1_train, _, state = module_call(term, 2)
    assert R.same_bits(loss_eval, loss_train) and R.same_bits(g1_eval, g1_train) and float(state[2]) == 3.0
    assert not R.same_bits(state[4:6], moved[4:6])
    # state_dict round trip: into a fresh module, in place
    saved = {k: v.cpu().clone() for k, v in term.state_dict().items()}
    assert list(saved) == ["noise_state"]
    fresh = make_term(sigma=0.3, gain=0.5)
    fresh_address = fresh.noise_state.data_ptr()
    fresh.load_state_dict(saved)
    assert R.same_bits(fresh.noise_state.cpu(), state) and fresh.noise_state.data_ptr() == fresh_address
    assert term.noise_state.data_ptr() == address and fresh.noise_state.is_cuda
    assert fresh.estimated_gain() == float(state[4])
    a, b = module_call(term, 3), module_call(fresh, 3)
    assert all(R.same_bits(u, v) for u, v in zip(a, b))
    # no gradient reaches the state; one entry point per call
    assert term.noise_state.grad is None and not term.noise_state.requires_grad
    N = native()
    y, y1, y2, b_ = (t.cuda() for t in U.trajectory_inputs(0))
    N.record_calls(True)
    term(y=y, x_net=None, physics=None, model=None, b=b_, y1=y1, y2=y2)
    calls = N.record_calls(False)
    assert [c[0] for c in calls] == ["sei_sure_loss_unsure_pg"] and len(calls[0][1]) == 21


# ------------------------------------------------------------------------------------------------ 6. replay equals eager
def ref_args(**over):
    import bench
    a = bench.reference_args("cuda", hidden=8, scales=3)
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("method", ["proposed", "sure"])
def test_replayed_steps_equal_eager_steps(method):
    """tests/test_unsure_gpu.py's step test on synthetic Poisson-Gaussian measurements: the small U-Net, batch 4, 48 x 48
    crops, four steps (zero_grad + loss + backward; the weights stay put, so the multipliers are what moves) with equal
    seeds, eagerly and through GraphedLossStep: the losses and all eight state floats bit for bit. Building the
    GraphedLossStep -- three warm-up steps on a zero measurement, then the capture -- leaves noise_state as it found it."""
    import models
    import physics
    from graphs import GraphedLossStep
    from losses import get_loss
    from optim import FlatAdam
    from physics._base import PoissonGaussianNoise
    args = ref_args(method=method, sure_unknown_noise=True, unsure_noise_model="poisson_gaussian",
                    unsure_init_noise_level=15.0, unsure_init_gain=0.02, unsure_step_size=1e-3, unsure_gain_step_size=2e-3,
                    noise_gain=0.01)
    p = physics.get_physics(args, "cuda")
    assert type(p.noise_model) is PoissonGaussianNoise
    torch.manual_seed(0)
    model = models.get_model(args, p, "cuda").to("cuda")
    model.train()
    lf = get_loss(args, p).to("cuda")
    term = lf.unsure_term()
    start = term.noise_state.cpu().clone()
    assert R.same_bits(start, torch.tensor(pg_state((15 / 255) ** 2, 0.02), dtype=F32))
    opt = FlatAdam(model, lr=1e-4)
    x = torch.rand(4, 3, 256, 256, device="cuda")
    y = p(x)
    assert y.shape == x.shape and bool(torch.isfinite(y).all())
    address = term.noise_state.data_ptr()
    graphed = GraphedLossStep(lf, model, opt, (4, 3, 48, 48))
    torch.cuda.synchronize()
    assert R.same_bits(term.noise_state.cpu(), start) and term.noise_state.data_ptr() == address
    bb = model.get_backbone()
    runs = {}
    for mode in ("graph", "eager"):
        term.noise_state.copy_(start)
        torch.manual_seed(21)                 # CPU generator: the crop offsets
        torch.cuda.manual_seed(22)            # device generator: probe, rates, centres, noise
        seq = []
        for _ in range(4):
            if mode == "graph":
                v = graphed(x, y)
            else:
                bb.zero_grad_flat()
                v = lf(x=x, y=y, model=model)
                v.backward()
            seq.append((v.detach().cpu().clone(), term.noise_state.cpu().clone()))
        runs[mode] = seq
    for i, ((lg, sg), (le, se)) in enumerate(zip(runs["graph"], runs["eager"])):
        print(f"{method} step {i + 1}: loss replay {float(lg)!r} eager {float(le)!r}; state replay {sg.tolist()} "
              f"eager {se.tolist()}")
    for (lg, sg), (le, se) in zip(runs["graph"], runs["eager"]):
        assert R.same_bits(lg, le) and R.same_bits(sg, se)
    states = [s for _, s in runs["graph"]]
    assert [float(s[2]) for s in states] == [1.0, 2.0, 3.0, 4.0]
    for slot in (0, 4):
        assert len({float(s[slot]) for s in states} | {float(start[slot])}) == 5, "both multipliers move every step"
    assert all(np.isfinite(float(v)) for v, _ in runs["graph"])


# ------------------------------------------------------------------------------------------------ 7. train.py end to end
def train_cmd(out, *extra):
    return [sys.executable, os.path.join(ROOT, "train.py"), "--device", "cuda", "--task", "deblurring", "--kernel",
            "Gaussian_R2", "--ProposedModel__architecture", "Convolutional", "--ConvolutionalModel__hidden_channels", "8",
            "--ConvolutionalModel__scales", "3", "--dataset", "synthetic", "--batch_size", "2", "--epochs", "2",
            "--max_steps", "2", "--lr_scheduler_kind", "multi_step_decay", "--noise_level", "5", "--noise_gain", "0.01",
            "--method", "proposed", "--sure_unknown_noise",
            "--unsure_noise_model", "poisson_gaussian", "--unsure_init_noise_level", "15", "--unsure_init_gain", "0.02",
            "--out_dir", str(out)] + list(extra)


def run_train(cmd, check=True):
    env = dict(os.environ, SEI_TRACE_STEP_KIND="1", SEI_TRACE_UNSURE_STATE="1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    if check:
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def traced_state(stdout):
    found = {}
    for prefix in ("unsure state at start:", "unsure gain state at start:"):
        words = next(ln for ln in stdout.splitlines() if ln.startswith(prefix)).split()
        found.update({w: float(words[i + 1]) for i, w in enumerate(words) if w in ("eta", "m", "k", "gamma", "m_gamma")})
    return [found[k] for k in ("eta", "m", "k", "gamma", "m_gamma")]


def test_train_script_with_unknown_poisson_gaussian_noise(tmp_path):
    """Two epochs of two steps at tests/test_unsure_gpu.py's smallest configuration, the synthetic measurements
    Poisson-Gaussian: a replayed step, four finite csv columns, the eight-float state in the checkpoints, restored by
    --RESUME; a checkpoint whose loss_state has the Gaussian length is refused with both lengths named."""
    out = tmp_path / "run"
    stdout = run_train(train_cmd(out)).stdout
    assert "step kind: hipGraph replay" in stdout, stdout
    eta0, gamma0 = float(L.f32((15 / 255) ** 2)), float(L.f32(0.02))
    assert traced_state(stdout) == [eta0, 0.0, 0.0, gamma0, 0.0]
    rows = open(out / "training.csv").read().strip().splitlines()
    assert rows[0] == "Epoch,Training Loss,Estimated Noise Level,Estimated Noise Gain" and len(rows) == 3
    values = [[float(v) for v in r_.split(",")] for r_ in rows[1:]]
    assert all(len(v) == 4 and all(np.isfinite(v)) for v in values)
    assert values[0][2] != 15.0 and values[0][3] != 0.02 and values[1][2:] != values[0][2:]
    assert "Estimated_Noise_Level:" in stdout and "Estimated_Noise_Gain:" in stdout
    ckp = torch.load(out / "checkpoints" / "ckp_2.pt", map_location="cpu")
    assert set(ckp) == {"epoch", "params", "optimizer", "scheduler", "loss_state"}
    state = ckp["loss_state"]["noise_state"]
    assert state.numel() == 8 and float(state[2]) == 4.0 and R.same_bits(state[[3, 6, 7]], torch.zeros(3))
    assert abs(255 * max(float(state[0]), 0) ** 0.5 - values[1][2]) <= 1e-4 * values[1][2]
    assert float(state[4]) == pytest.approx(values[1][3], rel=1e-6)
    first = torch.load(out / "checkpoints" / "ckp_0.pt", map_location="cpu")["loss_state"]["noise_state"]
    assert R.same_bits(first, torch.tensor(pg_state(eta0, gamma0), dtype=F32))
    # --RESUME starts from the stored state (and counts on from its k)
    out2 = tmp_path / "run2"
    stdout = run_train(train_cmd(out2, "--RESUME", str(out / "checkpoints" / "ckp_2.pt"), "--lr", "1e-5")).stdout
    assert traced_state(stdout) == [float(state[0]), float(state[1]), 4.0, float(state[4]), float(state[5])]
    resumed = torch.load(out2 / "checkpoints" / "ckp_2.pt", map_location="cpu")["loss_state"]["noise_state"]
    assert float(resumed[2]) == 8.0
    # a Gaussian-length loss_state is refused by name, before any step
    ckp["loss_state"]["noise_state"] = state[:4].clone()
    short = tmp_path / "gaussian_length.pt"
    torch.save(ckp, short)
    r = run_train(train_cmd(tmp_path / "run3", "--RESUME", str(short), "--lr", "1e-5"), check=False)
    assert r.returncode != 0 and "step kind" not in r.stdout
    message = next(ln for ln in r.stderr.splitlines() if ln.startswith("ValueError"))
    assert "--unsure_noise_model" in message and "holds 4 floats" in message and "holds 8" in message, r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ 8. PoissonGaussianNoise
def test_poisson_gaussian_noise_statistics():
    """A x = 0.5 on 2^18 pixels, gain 0.01, sigma 0.02: z = gain Poisson(50) + sigma N(0, 1) has mean 0.5, variance
    v = gain^2 50 + sigma^2 = gain 0.5 + sigma^2 and fourth central moment mu4 = gain^4 (50 + 3 50^2) + 6 gain^2 50 sigma^2 +
    3 sigma^4 (independent parts; Poisson: lambda + 3 lambda^2, normal: 3 sigma^4). The sample mean has standard error
    sqrt(v / n), the unbiased sample variance sqrt((mu4 - v^2 (n - 3) / (n - 1)) / n): both stay within 6 of them."""
    from physics._base import GaussianNoise, PoissonGaussianNoise
    n, gain, sigma, lam = 2 ** 18, 0.01, 0.02, 50.0
    x = torch.full((1, 1, 512, 512), 0.5, device="cuda")
    torch.manual_seed(1234)
    torch.cuda.manual_seed(1234)
    z = PoissonGaussianNoise(sigma=sigma, gain=gain)(x).double().cpu().reshape(-1)
    assert z.numel() == n
    v = gain ** 2 * lam + sigma ** 2
    assert abs(v - (gain * 0.5 + sigma ** 2)) < 1e-15
    mu4 = gain ** 4 * (lam + 3 * lam ** 2) + 6 * gain ** 2 * lam * sigma ** 2 + 3 * sigma ** 4
    se_mean, se_var = (v / n) ** 0.5, ((mu4 - v ** 2 * (n - 3) / (n - 1)) / n) ** 0.5
    mean, var = float(z.mean()), float(z.var(unbiased=True))
    print(f"PoissonGaussianNoise: mean {mean!r} ({(mean - 0.5) / se_mean:+.2f} standard errors of {se_mean:.2e}), variance "
          f"{var!r} against {v!r} ({(var - v) / se_var:+.2f} standard errors of {se_var:.2e})")
    assert abs(mean - 0.5) <= 6 * se_mean and abs(var - v) <= 6 * se_var
    # what the generator draws NEXT does not overlap with the Poisson sampler's counters: uncorrelated with this sample
    # (torch.poisson alone leaves a correlation of -0.07 at this rate on ROCm; 6 standard errors are 0.012)
    after = torch.randn_like(x).double().cpu().reshape(-1)
    corr = float(((z - z.mean()) * (after - after.mean())).mean() / (z.std() * after.std()))
    print(f"PoissonGaussianNoise: correlation with the next normal draw {corr:+.4f} (standard error {n ** -0.5:.4f})")
    assert abs(corr) <= 6 * n ** -0.5
    # the counts are there: without the Gaussian part the values are multiples of the gain
    torch.cuda.manual_seed(7)
    counts_only = PoissonGaussianNoise(sigma=0.0, gain=gain)(x).double().cpu() / float(L.f32(gain))
    assert float((counts_only - counts_only.round()).abs().max()) < 1e-3 and float(counts_only.min()) >= 0
    # gain = 0 is the Gaussian path: the same draws, the same bits; negative signals are clamped under the Poisson draw
    xr = torch.rand(2, 3, 17, 9, device="cuda")
    torch.cuda.manual_seed(99)
    plain = GaussianNoise(sigma=sigma)(xr)
    torch.cuda.manual_seed(99)
    assert R.same_bits(PoissonGaussianNoise(sigma=sigma, gain=0.0)(xr), plain)
    assert bool(torch.isfinite(PoissonGaussianNoise(sigma=sigma, gain=gain)(xr - 0.5)).all())
