"""SURE loss for Gaussian noise with a Monte-Carlo divergence (reference: src/losses/sure.py).

    loss = mean_int((A(x_net) - y)^2) + 2 sigma^2 * mean_int(b * (A(f(y + tau b)) - A(x_net)) / tau) - cst

`int` = the interior [m:-m, m:-m] of every image (m = `margin`; the divergence uses it only with
`cropped_div`), b ~ N(0,1) on that interior and 0 outside, cst = sigma^2 (averaged_cst) or
sigma^2 / batch_size. The two interior reductions and both gradients come out of one fused HIP kernel
(`sei_sure_terms`); the probe y + tau*b is `sei_axpy`.

`SureGaussianLoss(unsure=True)` is the same term for an UNKNOWN noise level (UNSURE; restated from the paper, see the
constructor): sigma^2 becomes a multiplier in device memory that `sei_sure_loss_unsure` reads and moves by gradient ascent.
`SurePoissonGaussianLoss` is that term for Poisson-Gaussian noise, variance sigma^2 + gain * signal with both levels unknown:
two multipliers, the weight eta + gamma y inside the divergence (`sei_sure_loss_unsure_pg`).
"""
import torch
import torch.nn as nn

import _native as N
from physics._ops import axpy


def _terms_buffers(ctx, y, y1, y2, b, margin_div, margin_mse, nsums=2):
    """What the SURE entry points take: the operands checked, the outputs and the gradients allocated and saved on `ctx`.
    -> (n_div, n_mse, out, work, (y1, y2, g1, g2 pointers)); `out` holds the `nsums` sums and the loss value behind them."""
    joint = y2 is None
    B, C, H, W = y.shape
    for name, t in (("y", y), ("y1", y1), ("b", b)) + (() if joint else (("y2", y2),)):
        N.check_tensor(t, name)
        if t.shape != ((2 * B, C, H, W) if joint and name == "y1" else y.shape):
            raise ValueError("SURE: y, A(x_net), A(f(y + tau b)) and b must share one shape")
    n_div = B * C * (H - 2 * margin_div) * (W - 2 * margin_div)
    n_mse = B * C * (H - 2 * margin_mse) * (W - 2 * margin_mse)
    out = torch.empty(nsums + 1, dtype=torch.float32, device=y.device)
    work = torch.empty(nsums * N.SEI_REDUCE_BLOCKS, dtype=torch.float32, device=y.device)
    if joint:
        g = torch.empty_like(y1)
        half = y.numel() * y.element_size()
        ptrs = (y1.data_ptr(), y1.data_ptr() + half, g.data_ptr(), g.data_ptr() + half)
        ctx.save_for_backward(g)
    else:
        g1, g2 = torch.empty_like(y), torch.empty_like(y)
        ptrs = (y1.data_ptr(), y2.data_ptr(), g1.data_ptr(), g2.data_ptr())
        ctx.save_for_backward(g1, g2)
    ctx.joint = joint
    return n_div, n_mse, out, work, ptrs


def _scaled_terms_grads(ctx, go, nargs):
    """The saved gradients times the incoming one, in the places of y1 (and y2) among `nargs` forward arguments."""
    if ctx.joint:
        (g,) = ctx.saved_tensors
        return (None, N.scale_by(g, go)) + (None,) * (nargs - 2)
    g1, g2 = ctx.saved_tensors
    return (None, N.scale_by(g1, go), N.scale_by(g2, go)) + (None,) * (nargs - 3)


class _SureTerms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, y1, y2, b, margin_div, margin_mse, tau, sigma2, cst):
        """y2 None: `y1` is [A(x_net); A(f(y + tau b))] as ONE tensor of 2B images (ProposedLoss evaluates the operator on both
        model outputs at once): its halves are read in place and one gradient tensor comes back for it -- autograd then has
        no slices to differentiate (two zero fills, two copies and an add per step). The loss value
        c_mse * mse_sum + c_div * div_sum - cst is formed by the kernel's own last stage (sei_sure_loss)."""
        B, C, H, W = y.shape
        n_div, n_mse, out, work, ptrs = _terms_buffers(ctx, y, y1, y2, b, margin_div, margin_mse)
        c_mse, c_div = 1.0 / n_mse, 2.0 * sigma2 / n_div
        N.call("sei_sure_loss", y.data_ptr(), ptrs[0], ptrs[1], b.data_ptr(), B * C, H, W, margin_div, margin_mse, tau,
               c_mse, c_div, float(cst), out.data_ptr(), ptrs[2], ptrs[3], work.data_ptr())
        return out[2]

    @staticmethod
    def backward(ctx, go):
        return _scaled_terms_grads(ctx, go, 9)


class _UnsureTerms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, y1, y2, b, margin_div, margin_mse, tau, state, step_size, momentum, update):
        """_SureTerms with the multiplier eta = state[0] in device memory in the place of sigma^2 (sei_sure_loss_unsure):
        loss = c_mse * mse_sum + 2 eta * div_sum / n_div, the gradients carry eta as it stands on entry, and with `update`
        the kernel's last stage then moves `state` = {eta, m, k, unused} one ascent step, in place. No gradient reaches
        `state`: the multiplier is not a parameter of the descent."""
        B, C, H, W = y.shape
        N.check_tensor(state, "noise_state")
        if state.numel() != 4 or state.device != y.device:
            raise ValueError("UNSURE: noise_state must hold four floats on the device of y (move the loss module there)")
        n_div, n_mse, out, work, ptrs = _terms_buffers(ctx, y, y1, y2, b, margin_div, margin_mse)
        N.call("sei_sure_loss_unsure", y.data_ptr(), ptrs[0], ptrs[1], b.data_ptr(), B * C, H, W, margin_div, margin_mse,
               tau, 1.0 / n_mse, 1.0 / n_div, float(step_size), float(momentum), int(bool(update)), state.data_ptr(),
               out.data_ptr(), ptrs[2], ptrs[3], work.data_ptr())
        return out[2]

    @staticmethod
    def backward(ctx, go):
        return _scaled_terms_grads(ctx, go, 11)


class _UnsurePgTerms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, y1, y2, b, margin_div, margin_mse, tau, state, step_eta, step_gamma, momentum, update):
        """_UnsureTerms with the per-pixel weight eta + gamma y, eta = state[0] and gamma = state[4] in device memory
        (sei_sure_loss_unsure_pg): loss = c_mse * mse_sum + 2 (eta * div_sum + gamma * ydiv_sum) / n_div, the gradients carry
        both multipliers as they stand on entry, and with `update` the kernel's last stage then moves `state` =
        {eta, m_eta, k, 0, gamma, m_gamma, 0, 0} one ascent step each, in place. No gradient reaches `state`."""
        B, C, H, W = y.shape
        N.check_tensor(state, "noise_state")
        if state.numel() != 8 or state.device != y.device:
            raise ValueError("UNSURE: the Poisson-Gaussian noise_state must hold eight floats on the device of y (move the "
                             "loss module there)")
        n_div, n_mse, out, work, ptrs = _terms_buffers(ctx, y, y1, y2, b, margin_div, margin_mse, nsums=3)
        N.call("sei_sure_loss_unsure_pg", y.data_ptr(), ptrs[0], ptrs[1], b.data_ptr(), B * C, H, W, margin_div, margin_mse,
               tau, 1.0 / n_mse, 1.0 / n_div, float(step_eta), float(step_gamma), float(momentum), int(bool(update)),
               state.data_ptr(), out.data_ptr(), ptrs[2], ptrs[3], work.data_ptr())
        return out[3]

    @staticmethod
    def backward(ctx, go):
        return _scaled_terms_grads(ctx, go, 12)


def draw_probe(y, margin):
    """b: N(0,1) on the interior, 0 on the `margin`-wide border (reference mc_div, :9-22)."""
    if margin == 0:
        return torch.randn_like(y)
    b = torch.zeros_like(y)
    b[:, :, margin:-margin, margin:-margin] = torch.randn(
        y.size(0), y.size(1), y.size(2) - 2 * margin, y.size(3) - 2 * margin, device=y.device, dtype=y.dtype)
    return b


def embed_probe(y, b_interior, margin):
    """Zero-extend an interior-shaped draw to y's shape (for injected randomness in tests)."""
    if margin == 0:
        return b_interior.contiguous()
    b = torch.zeros_like(y)
    b[:, :, margin:-margin, margin:-margin] = b_interior
    return b


class SureGaussianLoss(nn.Module):
    def __init__(self, sigma, tau=1e-2, margin=0, cropped_div=False, averaged_cst=False, unsure=False, step_size=1e-4,
                 momentum=0.9):
        """unsure: the noise level is unknown (UNSURE, Tachella, Davies, Jacques; restated from the paper -- deepinv is
        not part of this tree, parity with its SureGaussianLoss(unsure=True) is unpinned). sigma^2 becomes a Lagrange
        multiplier eta that starts at `sigma`^2 and takes one step of gradient ascent per training-mode forward:

            loss = mean_int((A(x_net) - y)^2) + 2 eta d,   d = mean_int(b * (A(f(y + tau b)) - A(x_net)) / tau)
            g = 2 d;  m' = g on the first step, else momentum * m + (1 - momentum) * g;  eta' = eta + step_size * m'

        (no constant term; the update uses the averaged direction m'). The state {eta, m, k, unused} is the float32
        buffer `noise_state`: the kernels read and write it in device memory, so a captured step replays the update."""
        super().__init__()
        self.name = "SureGaussian"
        self.sigma2 = sigma**2
        self.tau = tau
        assert margin is not None
        self.margin = margin
        self.cropped_div = cropped_div
        self.averaged_cst = averaged_cst
        self.unsure = bool(unsure)
        if self.unsure:
            if not 0.0 <= momentum < 1.0:
                raise ValueError(f"UNSURE: momentum must lie in [0, 1), got {momentum}")
            self.step_size, self.momentum = float(step_size), float(momentum)
            self.register_buffer("noise_state", torch.tensor([self.sigma2, 0.0, 0.0, 0.0], dtype=torch.float32))

    @property
    def div_margin(self):
        return self.margin if self.cropped_div else 0

    def estimated_sigma(self):
        """sqrt(max(eta, 0)) as a host float: a synchronisation, for use outside the step only."""
        if not self.unsure:
            raise RuntimeError("estimated_sigma: this SURE term was built with a known noise level (unsure=False)")
        return max(float(self.noise_state[0]), 0.0) ** 0.5

    def _terms(self, y, y1, y2, b):
        if self.unsure:
            return _UnsureTerms.apply(y, y1, y2, b, self.div_margin, self.margin, self.tau, self.noise_state,
                                      self.step_size, self.momentum, self.training)
        cst = self.sigma2 if self.averaged_cst else self.sigma2 / y.size(0)
        return _SureTerms.apply(y, y1, y2, b, self.div_margin, self.margin, self.tau, self.sigma2, cst)

    def forward(self, y, x_net, physics, model, b=None, y1=None, y2=None, y12=None, **kwargs):
        """`b` (full-size probe), `y1` = A(x_net) and `y2` = A(model(y + tau b)) may be supplied by a
        caller that has already evaluated them (ProposedLoss batches the two network passes: `y12` = both as one
        tensor of 2B images)."""
        y = y.contiguous()
        if b is None:
            b = draw_probe(y, self.div_margin)
        if y12 is not None:
            loss = self._terms(y, y12.contiguous(), None, b)
        else:
            if y1 is None:
                y1 = physics.A(x_net)
            if y2 is None:
                y2 = physics.A(model(axpy(y, b, self.tau)))
            loss = self._terms(y, y1.contiguous(), y2.contiguous(), b)
        from os import environ
        if "_TEMPORARY_HOTFIX" in environ:       # reference :68-74
            assert physics.rate is not None
            return physics.rate**2 * loss
        return loss


class SurePoissonGaussianLoss(SureGaussianLoss):
    def __init__(self, sigma, gain=0.0, tau=1e-2, margin=0, cropped_div=False, averaged_cst=False, step_size=1e-4,
                 gain_step_size=None, momentum=0.9):
        """UNSURE for Poisson-Gaussian noise, variance sigma^2 + gain * (clean value) at a pixel, with BOTH levels unknown
        (the same paper's signal-dependent case; restated from it -- parity with deepinv's SurePGLoss(unsure=True) is
        unpinned). The multiplier becomes the affine weight eta + gamma y inside the divergence, one multiplier per
        zero-expected-divergence constraint, each with SureGaussianLoss(unsure=True)'s ascent step:

            loss = mean_int((A(x_net) - y)^2) + 2 (eta d0 + gamma d1)
            d0 = mean_int(b * (A(f(y + tau b)) - A(x_net)) / tau),   d1 = mean_int(y * b * (A(f(y + tau b)) - A(x_net)) / tau)
            per multiplier: g = 2 d;  m' = g on the first step, else momentum * m + (1 - momentum) * g;  value' = value + step * m'

        (no second-order term, no third model call). eta starts at `sigma`^2 and moves by `step_size`, gamma at `gain` by
        `gain_step_size` (default: `step_size`). The state {eta, m_eta, k, 0, gamma, m_gamma, 0, 0} is the float32 buffer
        `noise_state`, as the parent's: slots 0..2 keep their meaning."""
        super().__init__(sigma, tau=tau, margin=margin, cropped_div=cropped_div, averaged_cst=averaged_cst, unsure=True,
                         step_size=step_size, momentum=momentum)
        self.name = "SurePoissonGaussian"
        self.gain_step_size = self.step_size if gain_step_size is None else float(gain_step_size)
        self.noise_state = torch.tensor([self.sigma2, 0.0, 0.0, 0.0, float(gain), 0.0, 0.0, 0.0], dtype=torch.float32)

    def estimated_gain(self):
        """gamma as a host float, as it stands (not clamped): a synchronisation, for use outside the step only."""
        return float(self.noise_state[4])

    def _terms(self, y, y1, y2, b):
        return _UnsurePgTerms.apply(y, y1, y2, b, self.div_margin, self.margin, self.tau, self.noise_state, self.step_size,
                                    self.gain_step_size, self.momentum, self.training)
