"""A torch restatement of the UNSURE loss (SURE with an unknown noise level: Tachella, Davies, Jacques) for the tests of
losses/sure.py's SureGaussianLoss(unsure=True) and of sei_sure_loss_unsure. Restated from the paper; nothing of the library
under test is imported here, and deepinv is not part of this tree.

    loss = mean_int_m((y1 - y)^2) + 2 eta d,    d = mean_int_d(b (y2 - y1) / tau)
    g = 2 d;  m' = g on the first update, else mu m + (1 - mu) g;  eta' = eta + alpha m';  k' = k + 1

y1 = A(x_net), y2 = A(f(y + tau b)); int_m / int_d: the interiors [m : H - m, m : W - m] of every image for the two margins.
eta is a constant of the loss (the descent does not differentiate it) and moves by gradient ASCENT on d, along the averaged
direction m'. The loss is a plain torch expression and its gradients are autograd's; every function takes the float32 values
the product is handed as exact and evaluates them in `dtype` (torch.float64: the reference; torch.float32: the same chain,
whose deviation from float64 is the `ref32` of tests/streaming_ref.py's bars).

tests/test_unsure.py anchors `ascent` to closed forms on the CPU; tests/test_unsure_gpu.py holds the product to this module.
"""
import torch

import loss_reduction_ref as L

EPS32 = 2.0 ** -24           # half an ulp of a float32 value relative to it: one rounding


def unsure_loss(y, y1, y2, b, md, mm, tau, eta, dtype=torch.float64):
    """(loss, d, abs_d, mse) for (..., H, W) operands: abs_d is the mean of |b (y2 - y1) / tau| over the divergence interior, the
    size of what the divergence mean added up. `tau` is rounded to float32 first, as the C call rounds it; `eta` is taken as
    it is given."""
    H, W = y.shape[-2:]
    in_d, in_m = L.interior(H, W, md), L.interior(H, W, mm)
    y, b = y.to(dtype), b.to(dtype)
    y1, y2 = y1.to(dtype), y2.to(dtype)
    tau, eta = L.scalar(tau, dtype), torch.tensor(float(eta), dtype=dtype)
    terms = (b * (y2 - y1) / tau)[..., in_d]
    d = terms.mean()
    mse = ((y1 - y) ** 2)[..., in_m].mean()
    return mse + 2 * eta * d, d, terms.abs().mean(), mse


def unsure_loss_and_grads(y, y1, y2, b, md, mm, tau, eta, dtype=torch.float64):
    """-> dict(loss, d, abs_d, mse, g1, g2): the loss with autograd's gradients with respect to y1 and y2."""
    y1 = y1.detach().to(dtype).requires_grad_(True)
    y2 = y2.detach().to(dtype).requires_grad_(True)
    loss, d, abs_d, mse = unsure_loss(y, y1, y2, b, md, mm, tau, eta, dtype)
    g1, g2 = torch.autograd.grad(loss, [y1, y2])
    return dict(loss=loss.detach(), d=d.detach(), abs_d=abs_d.detach(), mse=mse.detach(), g1=g1, g2=g2)


def ascent(eta, m, k, d, alpha, mu):
    """One update of the multiplier's state from the divergence mean `d` (Python floats, float64 arithmetic)."""
    m = 2 * d if k == 0 else mu * m + (1 - mu) * 2 * d
    eta = eta + alpha * m
    return eta, m, k + 1


def rounded(v):
    """A Python float as a C `float` argument holds it."""
    return float(L.f32(v))


def state_bar(eta, m_new, alpha):
    """The bar of one update's m' and eta' against `ascent` on the kernel's own divergence sum: 8 * 2^-24 of
    max(|eta|, |alpha m'|, |m'|), at most four float32 roundings each with a factor two of margin."""
    return 8 * EPS32 * max(abs(eta), abs(alpha * m_new), abs(m_new))


def trajectory_inputs(step, shape=(2, 3, 16, 16)):
    """y, y1, y2, b of one call of a trajectory (float32; loss_reduction_ref.sure_inputs' distributions on `shape`)."""
    gen = L._gen(step, *shape, 41)
    y = torch.rand(shape, generator=gen)
    y1 = y + 0.1 * torch.randn(shape, generator=gen)
    y2 = y1 + L.TAU * torch.randn(shape, generator=gen)
    return y, y1, y2, torch.randn(shape, generator=gen)


def trajectory(steps, margin, tau, eta0, alpha, mu, dtype=torch.float64, inputs=trajectory_inputs):
    """`steps` training-mode calls from the state {eta0, 0, 0}: a list of dicts (unsure_loss_and_grads' keys, evaluated with
    the multiplier as it stood BEFORE the call's update, plus eta, m, k AFTER it). The state is carried in Python floats
    (float64) whatever `dtype` the loss is evaluated in; alpha, mu and eta0 are rounded to float32 first."""
    eta, m, k = rounded(eta0), 0.0, 0
    alpha, mu = rounded(alpha), rounded(mu)
    out = []
    for step in range(steps):
        y, y1, y2, b = inputs(step)
        r = unsure_loss_and_grads(y, y1, y2, b, margin, margin, tau, eta, dtype)
        eta, m, k = ascent(eta, m, k, float(r["d"]), alpha, mu)
        out.append(dict(r, eta=eta, m=m, k=k))
    return out
