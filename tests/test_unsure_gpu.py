"""UNSURE on the GPU: sei_sure_loss_unsure and sei_axpy_sqrt_dev through the C ABI, SureGaussianLoss(unsure=True), a
replayed step against an eager one, and train.py --sure_unknown_noise end to end.

Bars. The two sums, the loss value, g1 and g2 of the kernel grid: tests/test_loss_reductions_gpu.py's bars of sei_sure_loss,
max(5e-6, 3 * ref32) of float64 (sums and loss relative to the float64 sum of the absolute terms), against
loss_reduction_ref.sure with the constant term removed and c_div = 2 eta / n_div; g2 is not bit for bit here, because its
coefficient (2 eta) * inv_n_div is formed in float32 on the device. The state update: unsure_ref.ascent in float64 on the
kernel's OWN div sum, m' and eta' within 8 * 2^-24 of max(|eta|, |alpha m'|, |m'|) (at most four float32 roundings each:
d = div * inv_n_div, 1 - mu, (1 - mu) g, the fused mu m + ..; then the fused eta + alpha m'). sei_axpy_sqrt_dev: 2 ulp of
the float64 result (below). The module's trajectory: the per-step bars above against tests/unsure_ref.py's restatement,
times K for the state after K steps (test_module_trajectory states how the two per-step bars add). Replay against eager:
equality.

Measured on one MI355X (largest over the cases of a family):
    family                               ref32     bar        HIP deviation
    unsure div sum  (of sum |terms|)     8.0e-8    5.0e-6     8.0e-8
    unsure mse sum                       1.2e-7    5.0e-6     4.8e-8
    unsure loss value (of its scale)     7.7e-8    5.0e-6     5.8e-8
    unsure g1                            1.1e-7    5.0e-6     1.7e-7
    unsure g2                            1.1e-7    5.0e-6     1.5e-7
    m' after one update (of the bar)     --        1.0        0.060
    eta' after one update (of the bar)   --        1.0        0.082
    sei_axpy_sqrt_dev (ulp of result)    --        2.0        0.519
    trajectory, 6 steps: eta (of bar)    --        1.0        0.0035
    trajectory, 6 steps: m (of bar)      --        1.0        0.0008
    trajectory, per step: loss           4.7e-8    5.0e-6     4.1e-8
    trajectory, per step: y1.grad        1.1e-7    5.0e-6     1.7e-7
    trajectory, per step: y2.grad        9.0e-8    5.0e-6     1.5e-7
(The trajectory's state bars are wide because they carry the floor of the divergence mean, 5e-6 of mean|terms|, every step;
the update itself is the tight check two rows above.) Replayed against eager steps: equal bits, --method proposed and sure.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import loss_reduction_ref as L
import streaming_ref as R
import unsure_ref as U

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
BLOCKS = 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ETA0 = float(L.f32(L.SIGMA ** 2))

# loss_reduction_ref.SURE_CASES entries, as (planes, H, W, margin_div, margin_mse): the smallest at which each path exists
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
    """A Guarded output whose first element lies `lead` floats behind the front margin (tests/test_loss_reductions_gpu.py)."""

    def __init__(self, shape, lead=0):
        n = int(torch.Size(shape if isinstance(shape, (tuple, list)) else (shape,)).numel())
        self.guard, self.lead = R.Guarded(n + lead), lead
        self.view = self.guard.view[lead:].view(shape)

    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        return self.guard.intact() and bool((self.guard.view[:self.lead] == R.SENTINEL).all())


def constants(case):
    planes, H, W, md, mm, _ = case
    n_div, n_mse = planes * (H - 2 * md) * (W - 2 * md), planes * (H - 2 * mm) * (W - 2 * mm)
    return 1.0 / n_mse, 1.0 / n_div, n_div


def run_unsure(case, state, alpha=1e-2, mu=0.9, update=1, tau=L.TAU, joint=False, lead=0):
    """One call on fresh buffers -> (out3, g1, g2, state after) on the CPU, the margins checked. `state`: four floats."""
    N = native()
    planes, H, W, md, mm, _ = case
    y, y1, y2, b = L.sure_inputs(*case)
    c_mse, inv_n_div, _ = constants(case)
    put = (lambda t: R.nan_framed(t, lead)) if lead else R.nan_tailed
    yd, bd = put(y), put(b)
    if joint:
        y12 = put(torch.stack([y1, y2]))
        g12 = Out((2, planes, H, W), lead)
        p1, p2, q1, q2, outs = y12[0].data_ptr(), y12[1].data_ptr(), g12.view[0].data_ptr(), g12.view[1].data_ptr(), [g12]
        assert p2 - p1 == 4 * y.numel() and q2 - q1 == 4 * y.numel()
    else:
        y1d, y2d, g1, g2 = put(y1), put(y2), Out((planes, H, W), lead), Out((planes, H, W), lead)
        p1, p2, q1, q2, outs = y1d.data_ptr(), y2d.data_ptr(), g1.ptr(), g2.ptr(), [g1, g2]
    assert not lead or all(p % 16 == 4 * lead for p in (yd.data_ptr(), bd.data_ptr(), p1, q1))
    out, work, st = Out(3, lead), Out(2 * BLOCKS, lead), R.Guarded(4)
    st.view.copy_(torch.tensor(state, dtype=F32))
    assert st.ptr() % 16 == 0
    N.call("sei_sure_loss_unsure", yd.data_ptr(), p1, p2, bd.data_ptr(), planes, H, W, md, mm, tau, c_mse, inv_n_div,
           alpha, mu, update, st.ptr(), out.ptr(), q1, q2, work.ptr())
    torch.cuda.synchronize()
    assert out.intact() and work.intact() and st.intact() and all(g.intact() for g in outs), case
    assert R.same_bits(yd, y) and R.same_bits(bd, b)
    if joint:
        return out.view.cpu(), g12.view[0].cpu(), g12.view[1].cpu(), st.view.cpu()
    return out.view.cpu(), g1.view.cpu(), g2.view.cpu(), st.view.cpu()


def references(case, eta, tau=L.TAU):
    planes, H, W, md, mm, _ = case
    c_mse, _, n_div = constants(case)
    inp = L.sure_inputs(*case)
    return tuple(L.sure(*inp, md, mm, tau, c_mse, 2.0 * eta / n_div, 0.0, dt) for dt in (F64, F32))


def hold_terms(label, got, r64, r32):
    out, g1, g2 = got[:3]
    R.hold32_on(label + " div sum", out[0], r64["div"], r32["div"], r64["abs_div"])
    R.hold32_on(label + " mse sum", out[1], r64["mse"], r32["mse"], r64["mse"])
    R.hold32_on(label + " loss", out[2], r64["loss"], r32["loss"], r64["loss_scale"])
    R.hold32(label + " g1", g1, r64["g1"], r32["g1"])
    if float(r64["g2"].abs().max()) > 0:
        R.hold32(label + " g2", g2, r64["g2"], r32["g2"])
    assert bool((g2[r64["g2"] == 0] == 0).all()), label + ": g2 is zero outside the divergence interior"


def hold_state(label, case, before, after, div_sum, alpha, mu):
    """m', eta', k' against unsure_ref.ascent in float64 on the kernel's own div sum and the float32-rounded arguments."""
    _, inv_n_div, _ = constants(case)
    eta, m, k = (float(v) for v in before[:3])
    d = float(div_sum) * U.rounded(inv_n_div)
    e64, m64, k64 = U.ascent(eta, m, int(k), d, U.rounded(alpha), U.rounded(mu))
    bar = U.state_bar(eta, m64, U.rounded(alpha))
    dev_m, dev_e = abs(float(after[1]) - m64), abs(float(after[0]) - e64)
    print(f"{label}: m' {float(after[1])!r} (float64 {m64!r}, apart {dev_m:.2e}), eta' {float(after[0])!r} (float64 {e64!r}, "
          f"apart {dev_e:.2e}), bar {bar:.2e}: {dev_m / bar:.3f} and {dev_e / bar:.3f} of it")
    assert dev_m <= bar and dev_e <= bar, label
    assert float(after[2]) == k64 and R.same_bits(after[3:], torch.tensor(before[3:], dtype=F32)), label
    return e64, m64


# ------------------------------------------------------------------------------------------------ 1. kernel grid
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_kernel_grid(case):
    """Sums, loss and both gradients with eta = float32(SIGMA^2) in device memory, the first update riding along (the
    gradients carry the multiplier as it stood before it); called again on the same state, the same bits everywhere."""
    state = [ETA0, 0.0, 0.0, 0.0]
    r64, r32 = references(case, ETA0)
    got = run_unsure(case, state)
    hold_terms(f"unsure {ids(case)}", got, r64, r32)
    hold_state(f"unsure {ids(case)}", case, state, got[3], got[0][0], 1e-2, 0.9)
    again = run_unsure(case, state)
    assert all(R.same_bits(a, b) for a, b in zip(got, again))


# ------------------------------------------------------------------------------------------------ 2. state update
STATE_CASE = next(c for c in L.SURE_CASES if c[:5] == (3, 48, 48, 6, 6))


@pytest.mark.parametrize("label,state,alpha,mu", [
    ("first call, a stale m ignored", [ETA0, 3.0, 0.0, 0.0], 1e-2, 0.9),
    ("later call", [0.0123, 0.37, 4.0, 0.0], 1e-2, 0.9),
    ("later call, the default step", [0.0123, -0.05, 7.0, 0.0], 1e-4, 0.9),
    ("momentum 0", [0.0123, 0.37, 4.0, 0.0], 1e-2, 0.0),
    ("a fourth element is left alone", [0.0123, 0.37, 2.0, 42.0], 1e-2, 0.5)])
def test_state_update(label, state, alpha, mu):
    got = run_unsure(STATE_CASE, state, alpha=alpha, mu=mu)
    _, m64 = hold_state(label, STATE_CASE, state, got[3], got[0][0], alpha, mu)
    if state[2] == 0.0 or mu == 0.0:
        d32 = got[0][0] * L.f32(constants(STATE_CASE)[1])
        assert float(got[3][1]) == float(2 * d32), "m' = g exactly: one rounding, the kernel's own"
    hold_terms(label, got, *references(STATE_CASE, state[0]))


def test_negative_divergence_takes_eta_below_zero_unclamped():
    """The sign of tau flips the divergence sum: with the one that makes it negative and a large step eta' < 0, stored as
    it is. (sqrt(max(eta, 0)) is the readers' business: estimated_sigma and sei_axpy_sqrt_dev.)"""
    case = CASES[1]                        # 1 x 5 x 9: a divergence mean of a quarter of its absolute terms' (the float64 figures)
    state, alpha = [ETA0, 0.0, 0.0, 0.0], 1.0
    r64 = references(case, ETA0)[0]
    assert abs(float(r64["div"])) > 0.2 * float(r64["abs_div"])
    tau = L.TAU if float(r64["div"]) < 0 else -L.TAU
    got = run_unsure(case, state, alpha=alpha, tau=tau)
    assert float(got[0][0]) < 0
    e64, _ = hold_state("negative div sum", case, state, got[3], got[0][0], alpha, 0.9)
    assert e64 < -0.1 and float(got[3][0]) < -0.1
    hold_terms("negative div sum", got, *references(case, ETA0, tau))
    # the next call works with the negative multiplier as it stands
    after = [float(v) for v in got[3]]
    nxt = run_unsure(case, after, alpha=1e-3, tau=tau)
    hold_terms("negative eta", nxt, *references(case, after[0], tau))
    hold_state("negative eta", case, after, nxt[3], nxt[0][0], 1e-3, 0.9)


@pytest.mark.parametrize("case", [CASES[1], CASES[4], CASES[6]], ids=ids)
def test_update_0_leaves_the_state_bitwise_and_everything_else_the_same(case):
    state = [0.0123, 0.37, 4.0, -0.0]
    frozen, moved = run_unsure(case, state, update=0), run_unsure(case, state, update=1)
    assert R.same_bits(frozen[3], torch.tensor(state, dtype=F32))
    assert not R.same_bits(moved[3], frozen[3])
    assert all(R.same_bits(a, b) for a, b in zip(frozen[:3], moved[:3]))


def test_joint_layout_and_storage_offset():
    """y1 | y2 and g1 | g2 as the halves of one 2B-image tensor (ProposedLoss's fused pass), and every operand, output and
    the workspace 4 bytes off the 16-byte grid (the state keeps its own alignment): the plain aligned call's bits."""
    state = [0.0123, 0.37, 4.0, 0.0]
    joint_case, offset_case = L.SURE_JOINT, L.SURE_OFFSET
    for case, kw in ((joint_case, dict(joint=True)), (offset_case, dict(lead=1)), (joint_case, dict(joint=True, lead=1))):
        got, plain = run_unsure(case, state, **kw), run_unsure(case, state)
        hold_terms(f"unsure {ids(case)} {kw}", got, *references(case, state[0]))
        assert all(R.same_bits(a, b) for a, b in zip(got, plain)), kw


def test_refusals_touch_nothing():
    """Each refusal returns 10001 (SEI_ERR_BAD_ARG) and neither out3 nor the state nor anything else is written."""
    N = native()
    fn = N.lib().sei_sure_loss_unsure
    H, W = 8, 6
    t = R.nan_tailed(torch.rand((2, H, W)))
    out, g1, g2, work, st = R.Guarded(3), R.Guarded((2, H, W)), R.Guarded((2, H, W)), R.Guarded(2 * BLOCKS), R.Guarded(4)
    ok = dict(y=t.data_ptr(), y1=t.data_ptr(), y2=t.data_ptr(), b=t.data_ptr(), planes=2, H=H, W=W, md=2, mm=2, tau=0.01,
              c_mse=0.01, inv_n_div=0.02, step=1e-2, mu=0.9, update=1, state=st.ptr(), out3=out.ptr(), g1=g1.ptr(),
              g2=g2.ptr(), work=work.ptr(), stream=N.stream())
    bad = [dict(state=None), dict(state=st.ptr() + 4), dict(state=st.ptr() + 8), dict(mu=-0.1), dict(mu=1.0), dict(mu=1.5),
           dict(mu=float("nan")), dict(step=float("inf")), dict(step=float("-inf")), dict(step=float("nan")),
           # what sei_sure_loss refuses: an empty interior for either margin on either axis, tau == 0, planes == 0, a null
           dict(md=3, mm=0), dict(md=0, mm=3), dict(H=W, W=H, md=3, mm=0), dict(H=W, W=H, md=0, mm=3), dict(H=H, W=H, md=4, mm=4),
           dict(tau=0.0), dict(planes=0), dict(y=None), dict(b=None), dict(out3=None), dict(g2=None), dict(work=None)]
    for change in bad:
        assert fn(*dict(ok, **change).values()) == 10001, change
        torch.cuda.synchronize()
        for g in (out, g1, g2, work, st):
            assert g.intact() and bool((g.view == R.SENTINEL).all()), change
    st.view.copy_(torch.tensor([ETA0, 0.0, 0.0, 0.0]))
    assert fn(*ok.values()) == 0                                        # the same buffers, inside every bound
    torch.cuda.synchronize()
    assert bool((g1.view != R.SENTINEL).all()) and bool((out.view != R.SENTINEL).all()) and float(st.view[2]) == 1.0
    assert all(g.intact() for g in (out, g1, g2, work, st))


# ------------------------------------------------------------------------------------------------ 3. sei_axpy_sqrt_dev
AXPY_N = [1, 3, 255, 1025, L.CAP + 1]


def axpy_inputs(n, signed_a):
    """a in [1, 2] (signed_a: in [-1, 1]) and b ~ N(0, 1) cut off at +-4."""
    gen = L._gen(n, 53)
    a = 2 * torch.rand(n, generator=gen) - 1 if signed_a else 1 + torch.rand(n, generator=gen)
    return a, torch.randn(n, generator=gen).clamp(-4, 4)


def run_axpy_sqrt(a, b, p):
    N = native()
    ad, bd, pd, out = R.nan_tailed(a), R.nan_tailed(b), R.nan_tailed(torch.tensor([p], dtype=F32)), R.Guarded(a.numel())
    N.call("sei_axpy_sqrt_dev", ad.data_ptr(), bd.data_ptr(), pd.data_ptr(), out.ptr(), a.numel())
    torch.cuda.synchronize()
    assert out.intact() and R.same_bits(ad, a) and R.same_bits(bd, b) and float(pd[0]) == float(L.f32(p))
    return out.view.cpu()


def ulps_apart(got, r64):
    """|got - r64| in units of the float32 spacing at |r64| (at least the smallest subnormal), largest over the elements."""
    mag = r64.abs().float()
    ulp = (torch.nextafter(mag, torch.full_like(mag, float("inf"))) - mag).double()
    return float(((got.double() - r64).abs() / ulp).max())


@pytest.mark.parametrize("n", AXPY_N)
def test_axpy_sqrt_dev(n):
    """a + sqrt(max(p, 0)) b against float64 to 2 ulp of the result. The kernel rounds twice, the square root (half an ulp
    of s = sqrt(p), times |b|) and the fused multiply-add (half an ulp of the result r): (2^-24 |s b| + 2^-24 |r|) in all,
    which is within 2 ulp of r whenever |s b| <= 1.5 |r|. A bar relative to r can ask that of no implementation where
    s b cancels a, so the general case keeps them apart -- a in [1, 2], |b| <= 4, s <= 0.1: |s b| <= 0.4 <= |r| -- with a
    signed b and an s that float32 does not hold exactly; p = 1/16 (s = 1/4 exactly: the fused multiply-add alone rounds)
    runs on a signed a, cancellation and all. p = 0 and p < 0 return a bit for bit."""
    worst = 0.0
    for p, signed_a in ((ETA0, False), (float(L.f32(1e-4)), False), (0.0625, True)):
        a, b = axpy_inputs(n, signed_a)
        r64 = a.double() + torch.tensor(float(L.f32(p)), dtype=F64).sqrt() * b.double()
        got = run_axpy_sqrt(a, b, p)
        apart = ulps_apart(got, r64)
        print(f"axpy_sqrt_dev n={n} p={p!r}: {apart:.3f} ulp of the float64 result")
        worst = max(worst, apart)
    assert worst <= 2.0
    a, b = axpy_inputs(n, True)
    for p in (0.0, -0.0, -1e-3, -float("inf")):
        assert R.same_bits(run_axpy_sqrt(a, b, p), a), p


def test_axpy_sqrt_dev_refuses_misaligned_pointers():
    N = native()
    fn = N.lib().sei_axpy_sqrt_dev
    a, b, p = R.nan_tailed(torch.rand(16)), R.nan_tailed(torch.rand(16)), R.nan_tailed(torch.tensor([0.01]))
    out = R.Guarded(16)
    ok = [a.data_ptr(), b.data_ptr(), p.data_ptr(), out.ptr(), 8, N.stream()]
    for i in (0, 1, 3):
        args = list(ok)
        args[i] += 4
        assert fn(*args) == 10001
    for args in ([None] + ok[1:], ok[:2] + [None] + ok[3:], ok[:4] + [0, ok[5]]):
        assert fn(*args) == 10001
    torch.cuda.synchronize()
    assert out.intact() and bool((out.view == R.SENTINEL).all())
    # the host layer stages an operand off the grid in a fresh allocation instead (physics/_ops.py), the same bits
    from physics._ops import axpy_sqrt_dev
    x, n_ = torch.rand(2, 3, 5, 5), torch.randn(2, 3, 5, 5)
    off = axpy_sqrt_dev(R.nan_framed(x, 1), R.nan_framed(n_, 3), p)
    assert R.same_bits(off, run_axpy_sqrt(x.reshape(-1), n_.reshape(-1), 0.01).view(x.shape))


# ------------------------------------------------------------------------------------------------ 4. module trajectory
TRAJ = dict(steps=6, margin=2, sigma=0.1, alpha=5e-3, mu=0.9)


def make_term(**over):
    from losses.sure import SureGaussianLoss
    kw = dict(sigma=TRAJ["sigma"], margin=TRAJ["margin"], cropped_div=True, unsure=True, step_size=TRAJ["alpha"],
              momentum=TRAJ["mu"])
    kw.update(over)
    return SureGaussianLoss(**kw).to("cuda")


def module_call(term, step):
    y, y1, y2, b = (t.cuda() for t in U.trajectory_inputs(step))
    y1.requires_grad_(True)
    y2.requires_grad_(True)
    loss = term(y=y, x_net=None, physics=None, model=None, b=b, y1=y1, y2=y2)
    loss.backward()
    return loss.detach().cpu(), y1.grad.cpu(), y2.grad.cpu(), term.noise_state.cpu().clone()


def test_module_trajectory():
    """Six training-mode calls on y1 / y2 given as autograd leaves at (2, 3, 16, 16), margin 2, against the float64 torch
    restatement (a plain expression, autograd's gradients, the update in three lines). Per step: loss to max(5e-6, 3 ref32)
    of |mse| + 2 |eta| mean|terms|, gradients to the same bar of their largest element. State after K steps: K times the
    per-step bar, which adds the two bars a step is held to -- the update's own, 8 * 2^-24 of max(|eta|, |alpha m'|, |m'|),
    and the divergence mean's, max(5e-6, 3 ref32) of mean|terms|, which enters m' through g = 2 d (a factor 2) and eta'
    through alpha m' (a factor 2 alpha). (m' averages the g's with weights that sum to one, so their deviations do not add
    up in it: K times the bar is ample there. eta' sums alpha m' over the steps: K times.)"""
    K, alpha = TRAJ["steps"], U.rounded(TRAJ["alpha"])
    args = (K, TRAJ["margin"], L.TAU, TRAJ["sigma"] ** 2, TRAJ["alpha"], TRAJ["mu"])
    r64, r32 = U.trajectory(*args, dtype=F64), U.trajectory(*args, dtype=F32)
    term = make_term()
    assert term.training and R.same_bits(term.noise_state.cpu(), torch.tensor([TRAJ["sigma"] ** 2, 0, 0, 0], dtype=F32))
    eta_before = float(term.noise_state[0])
    worst = {"eta": 0.0, "m": 0.0}
    for i in range(K):
        loss, g1, g2, state = module_call(term, i)
        a, c = r64[i], r32[i]
        eta64_before = U.rounded(TRAJ["sigma"] ** 2) if i == 0 else r64[i - 1]["eta"]
        scale = float(a["mse"]) + 2 * abs(eta64_before) * float(a["abs_d"])
        R.hold32_on(f"step {i + 1} loss", loss, a["loss"], c["loss"], scale)
        R.hold32(f"step {i + 1} y1.grad", g1, a["g1"], c["g1"])
        R.hold32(f"step {i + 1} y2.grad", g2, a["g2"], c["g2"])
        ref32_d = abs(float(c["d"]) - float(a["d"])) / float(a["abs_d"])
        step_bar = U.state_bar(eta_before, a["m"], alpha) + 2 * R.bar(ref32_d) * float(a["abs_d"])
        bar_m, bar_eta = (i + 1) * step_bar, (i + 1) * (U.state_bar(eta_before, a["m"], alpha) + alpha * step_bar)
        dev_m, dev_eta = abs(float(state[1]) - a["m"]), abs(float(state[0]) - a["eta"])
        print(f"step {i + 1}: eta {float(state[0])!r} (float64 {a['eta']!r}, apart {dev_eta:.2e}, bar {bar_eta:.2e}), "
              f"m {float(state[1])!r} (float64 {a['m']!r}, apart {dev_m:.2e}, bar {bar_m:.2e})")
        assert dev_m <= bar_m and dev_eta <= bar_eta and float(state[2]) == i + 1 == a["k"]
        worst = {"eta": max(worst["eta"], dev_eta / bar_eta), "m": max(worst["m"], dev_m / bar_m)}
        eta_before = float(state[0])
    print(f"trajectory: largest deviation {worst['eta']:.4f} (eta) and {worst['m']:.4f} (m) of the bars")
    assert float(term.noise_state[0]) != float(L.f32(TRAJ["sigma"] ** 2))
    assert abs(term.estimated_sigma() - max(float(term.noise_state[0]), 0.0) ** 0.5) == 0.0


def test_module_in_eval_mode_and_state_dict():
    term = make_term()
    for i in range(2):
        module_call(term, i)
    moved = term.noise_state.cpu().clone()
    assert float(moved[2]) == 2.0
    address = term.noise_state.data_ptr()
    term.eval()
    loss_eval, g1_eval, _, state = module_call(term, 2)
    assert R.same_bits(state, moved), "eval: the state does not move"
    term.train()
    loss_train, g1_train, _, state = module_call(term, 2)
    assert R.same_bits(loss_eval, loss_train) and R.same_bits(g1_eval, g1_train) and float(state[2]) == 3.0
    # state_dict round trip: into a fresh module, in place
    saved = {k: v.cpu().clone() for k, v in term.state_dict().items()}
    assert list(saved) == ["noise_state"]
    fresh = make_term(sigma=0.3)
    fresh_address = fresh.noise_state.data_ptr()
    fresh.load_state_dict(saved)
    assert R.same_bits(fresh.noise_state.cpu(), state) and fresh.noise_state.data_ptr() == fresh_address
    assert term.noise_state.data_ptr() == address and fresh.noise_state.is_cuda
    a, b = module_call(term, 3), module_call(fresh, 3)
    assert all(R.same_bits(u, v) for u, v in zip(a, b))
    # unsure=False: the entry point, its arguments and the number of launches of the parent
    from losses.sure import SureGaussianLoss
    N = native()
    plain = SureGaussianLoss(sigma=0.1, margin=2, cropped_div=True).to("cuda")
    assert dict(plain.named_buffers()) == {}
    y, y1, y2, b_ = (t.cuda() for t in U.trajectory_inputs(0))
    N.record_calls(True)
    plain(y=y, x_net=None, physics=None, model=None, b=b_, y1=y1, y2=y2)
    calls = N.record_calls(False)
    assert [c[0] for c in calls] == ["sei_sure_loss"] and len(calls[0][1]) == 17
    N.record_calls(True)
    term(y=y, x_net=None, physics=None, model=None, b=b_, y1=y1, y2=y2)
    assert [c[0] for c in N.record_calls(False)] == ["sei_sure_loss_unsure"]


# ------------------------------------------------------------------------------------------------ 5. replay equals eager
def ref_args(**over):
    import bench
    a = bench.reference_args("cuda", hidden=8, scales=3)
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("method", ["proposed", "sure"])
def test_replayed_steps_equal_eager_steps(method):
    """tests/test_loss_gpu.py's small U-Net, batch 4, 48 x 48 crops: four steps (zero_grad + loss + backward, what the graph
    holds; the weights stay put, so the multiplier is the one thing that moves) with equal seeds, eagerly and through
    GraphedLossStep: the losses and the (eta, m, k) sequences bit for bit. Building the GraphedLossStep -- three warm-up
    steps on a zero measurement, then the capture -- leaves noise_state bit for bit as it found it."""
    import models
    import physics
    from graphs import GraphedLossStep
    from losses import get_loss
    from optim import FlatAdam
    args = ref_args(method=method, sure_unknown_noise=True, unsure_init_noise_level=15.0, unsure_step_size=1e-3)
    p = physics.get_physics(args, "cuda")
    torch.manual_seed(0)
    model = models.get_model(args, p, "cuda").to("cuda")
    model.train()
    lf = get_loss(args, p).to("cuda")
    term = lf.unsure_term()
    start = term.noise_state.cpu().clone()
    assert R.same_bits(start, torch.tensor([(15 / 255) ** 2, 0, 0, 0], dtype=F32))
    opt = FlatAdam(model, lr=1e-4)
    x = torch.rand(4, 3, 256, 256, device="cuda")
    y = p(x)
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
    assert len({float(s[0]) for s in states} | {float(start[0])}) == 5, "the multiplier moves every step"
    assert all(np.isfinite(float(v)) for v, _ in runs["graph"])


# ------------------------------------------------------------------------------------------------ 6. train.py end to end
def train_cmd(out, *extra):
    return [sys.executable, os.path.join(ROOT, "train.py"), "--device", "cuda", "--task", "deblurring", "--kernel",
            "Gaussian_R2", "--ProposedModel__architecture", "Convolutional", "--ConvolutionalModel__hidden_channels", "8",
            "--ConvolutionalModel__scales", "3", "--dataset", "synthetic", "--batch_size", "2", "--epochs", "1",
            "--max_steps", "3", "--noise_level", "5", "--out_dir", str(out)] + list(extra)


def run_train(cmd):
    env = dict(os.environ, SEI_TRACE_STEP_KIND="1", SEI_TRACE_UNSURE_STATE="1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def traced_state(stdout):
    line = next(ln for ln in stdout.splitlines() if ln.startswith("unsure state at start:"))
    words = line.split()
    return [float(words[i + 1]) for i, w in enumerate(words) if w in ("eta", "m", "k")]


def test_train_script_fine_tuning_on_measurements_with_an_unknown_noise_level(tmp_path):
    """The case the flag is for: --fine_tuning on a folder of measured PNGs (nobody knows their noise level), fused SGD,
    the step replayed from a hipGraph, two epochs of two steps (three files, batch 2: the short batch runs eagerly on the
    same state)."""
    from PIL import Image
    folder = tmp_path / "measurements"
    folder.mkdir()
    rng = np.random.default_rng(0)
    for k in range(3):
        Image.fromarray(rng.integers(0, 256, size=(64, 64, 3), dtype=np.uint8)).save(folder / f"y{k}.png")
    out = tmp_path / "run"
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--device", "cuda", "--task", "deblurring", "--kernel",
           "Gaussian_R2", "--ProposedModel__architecture", "Convolutional", "--ConvolutionalModel__hidden_channels", "8",
           "--ConvolutionalModel__scales", "3", "--dataset", str(folder), "--PrepareTrainingPairs__crop_size", "64",
           "--batch_size", "2", "--epochs", "2", "--method", "proposed", "--fine_tuning", "--lr_scheduler_kind",
           "multi_step_decay", "--sure_unknown_noise", "--unsure_init_noise_level", "20", "--out_dir", str(out)]
    stdout = run_train(cmd)
    assert "step kind: hipGraph replay" in stdout and "Selected optimizer: SGD" in stdout, stdout
    rows = open(out / "training.csv").read().strip().splitlines()
    assert rows[0] == "Epoch,Training Loss,Estimated Noise Level" and len(rows) == 3
    levels = [float(r_.split(",")[2]) for r_ in rows[1:]]
    assert all(np.isfinite(v) for v in levels) and levels[0] != 20.0 and levels[1] != levels[0]
    state = torch.load(out / "checkpoints" / "ckp_2.pt", map_location="cpu")["loss_state"]["noise_state"]
    assert float(state[2]) == 4.0                       # a replayed and an eager step per epoch


@pytest.mark.parametrize("method", ["proposed", "sure"])
def test_train_script_with_an_unknown_noise_level(tmp_path, method):
    flags = ["--method", method, "--sure_unknown_noise", "--unsure_init_noise_level", "15"]
    out = tmp_path / "run"
    stdout = run_train(train_cmd(out, *flags))
    assert "step kind: hipGraph replay" in stdout, stdout
    assert traced_state(stdout) == [float(L.f32((15 / 255) ** 2)), 0.0, 0.0]
    rows = open(out / "training.csv").read().strip().splitlines()
    assert rows[0] == "Epoch,Training Loss,Estimated Noise Level" and len(rows) == 2
    epoch, loss, level = rows[1].split(",")
    assert np.isfinite(float(loss)) and np.isfinite(float(level)) and float(level) != 15.0 and abs(float(level) - 15) > 1e-6
    assert "Estimated_Noise_Level:" in stdout
    ckp = torch.load(out / "checkpoints" / "ckp_1.pt", map_location="cpu")
    assert set(ckp) == {"epoch", "params", "optimizer", "scheduler", "loss_state"}
    state = ckp["loss_state"]["noise_state"]
    assert float(state[2]) == 3.0 and abs(255 * max(float(state[0]), 0) ** 0.5 - float(level)) <= 1e-4 * float(level)
    first = torch.load(out / "checkpoints" / "ckp_0.pt", map_location="cpu")["loss_state"]["noise_state"]
    assert R.same_bits(first, torch.tensor([(15 / 255) ** 2, 0, 0, 0], dtype=F32))
    if method != "proposed":
        return
    # --RESUME starts from the stored state (and counts on from its k)
    out2 = tmp_path / "run2"
    stdout = run_train(train_cmd(out2, *flags, "--RESUME", str(out / "checkpoints" / "ckp_1.pt"), "--lr", "1e-5"))
    assert traced_state(stdout) == [float(state[0]), float(state[1]), 3.0]
    resumed = torch.load(out2 / "checkpoints" / "ckp_1.pt", map_location="cpu")["loss_state"]["noise_state"]
    assert float(resumed[2]) == 6.0
    # the same command without the flag: the parent's csv and checkpoint
    out3 = tmp_path / "run3"
    stdout = run_train(train_cmd(out3, "--method", method))
    assert "unsure state" not in stdout and "Estimated" not in stdout and "step kind: hipGraph replay" in stdout
    rows = open(out3 / "training.csv").read().strip().splitlines()
    assert rows[0] == "Epoch,Training Loss" and len(rows) == 2 and len(rows[1].split(",")) == 2
    assert set(torch.load(out3 / "checkpoints" / "ckp_1.pt", map_location="cpu")) == {"epoch", "params", "optimizer",
                                                                                      "scheduler"}
