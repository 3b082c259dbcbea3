"""A torch restatement of the Poisson-Gaussian UNSURE loss (SURE with unknown noise levels where the variance at a pixel is
sigma^2 + gain * signal: Tachella, Davies, Jacques) for the tests of losses/sure.py's SurePoissonGaussianLoss and of
sei_sure_loss_unsure_pg. Restated from the paper; nothing of the library under test is imported here, and deepinv is not part of
this tree.

    loss = mean_int_m((y1 - y)^2) + 2 (eta d0 + gamma d1)
    d0 = mean_int_d(b (y2 - y1) / tau)        d1 = mean_int_d(y b (y2 - y1) / tau)
    per multiplier: g = 2 d;  m' = g on the first update, else mu m + (1 - mu) g;  value' = value + alpha m';  k' = k + 1 once

y1 = A(x_net), y2 = A(f(y + tau b)); int_m / int_d: the interiors [m : H - m, m : W - m] of every image for the two margins.
eta and gamma are constants of the loss (the descent does not differentiate them); each moves by gradient ASCENT on its own
constraint. The loss is a plain torch expression and its gradients are autograd's; every function takes the float32 values
the product is handed as exact and evaluates them in `dtype` (torch.float64: the reference; torch.float32: the same chain,
whose deviation from float64 is the `ref32` of tests/streaming_ref.py's bars).

tests/test_unsure_pg.py anchors this module to closed forms on the CPU; tests/test_unsure_pg_gpu.py holds the product to it.
"""
import torch

import loss_reduction_ref as L
import unsure_ref as U


def pg_loss(y, y1, y2, b, md, mm, tau, eta, gamma, dtype=torch.float64):
    """(loss, d0, d1, abs_d0, abs_d1, mse) for (..., H, W) operands: abs_d0 / abs_d1 are the means of the absolute terms of d0
    / d1 over the divergence interior, the sizes of what the two means added up. `tau` is rounded to float32 first, as the C
    call rounds it; `eta` and `gamma` are taken as they are given."""
    H, W = y.shape[-2:]
    in_d, in_m = L.interior(H, W, md), L.interior(H, W, mm)
    y, b = y.to(dtype), b.to(dtype)
    y1, y2 = y1.to(dtype), y2.to(dtype)
    tau = L.scalar(tau, dtype)
    eta, gamma = torch.tensor(float(eta), dtype=dtype), torch.tensor(float(gamma), dtype=dtype)
    terms0 = (b * (y2 - y1) / tau)[..., in_d]
    terms1 = (y * (b * (y2 - y1) / tau))[..., in_d]
    d0, d1 = terms0.mean(), terms1.mean()
    mse = ((y1 - y) ** 2)[..., in_m].mean()
    return mse + 2 * (eta * d0 + gamma * d1), d0, d1, terms0.abs().mean(), terms1.abs().mean(), mse


def pg_loss_and_grads(y, y1, y2, b, md, mm, tau, eta, gamma, dtype=torch.float64):
    """-> dict(loss, d0, d1, abs_d0, abs_d1, mse, g1, g2): the loss with autograd's gradients with respect to y1 and y2."""
    y1 = y1.detach().to(dtype).requires_grad_(True)
    y2 = y2.detach().to(dtype).requires_grad_(True)
    loss, d0, d1, a0, a1, mse = pg_loss(y, y1, y2, b, md, mm, tau, eta, gamma, dtype)
    g1, g2 = torch.autograd.grad(loss, [y1, y2])
    return dict(loss=loss.detach(), d0=d0.detach(), d1=d1.detach(), abs_d0=a0.detach(), abs_d1=a1.detach(),
                mse=mse.detach(), g1=g1, g2=g2)


def ascent(state, d0, d1, alpha_eta, alpha_gamma, mu):
    """One update of (eta, m_eta, gamma, m_gamma, k) from the two divergence means (Python floats, float64 arithmetic): the
    Gaussian rule (unsure_ref.ascent) once per multiplier on its own mean, one counter."""
    eta, m_eta, gamma, m_gamma, k = state
    eta, m_eta, _ = U.ascent(eta, m_eta, k, d0, alpha_eta, mu)
    gamma, m_gamma, k = U.ascent(gamma, m_gamma, k, d1, alpha_gamma, mu)
    return eta, m_eta, gamma, m_gamma, k


def trajectory(steps, margin, tau, eta0, gamma0, alpha_eta, alpha_gamma, mu, dtype=torch.float64,
               inputs=U.trajectory_inputs):
    """`steps` training-mode calls from the state {eta0, 0, gamma0, 0, k = 0}: a list of dicts (pg_loss_and_grads' keys,
    evaluated with the multipliers as they stood BEFORE the call's update, plus eta, m_eta, gamma, m_gamma, k AFTER it). The
    state is carried in Python floats (float64) whatever `dtype` the loss is evaluated in; the step sizes, mu and the two
    starting values are rounded to float32 first."""
    state = (U.rounded(eta0), 0.0, U.rounded(gamma0), 0.0, 0)
    alpha_eta, alpha_gamma, mu = U.rounded(alpha_eta), U.rounded(alpha_gamma), U.rounded(mu)
    out = []
    for step in range(steps):
        y, y1, y2, b = inputs(step)
        r = pg_loss_and_grads(y, y1, y2, b, margin, margin, tau, state[0], state[2], dtype)
        state = ascent(state, float(r["d0"]), float(r["d1"]), alpha_eta, alpha_gamma, mu)
        out.append(dict(r, eta=state[0], m_eta=state[1], gamma=state[2], m_gamma=state[3], k=state[4]))
    return out
