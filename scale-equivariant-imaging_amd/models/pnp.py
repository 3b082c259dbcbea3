"""The PlugAndPlay baseline (reference: src/models/pnp.py): DPIR-style half-quadratic splitting around a pretrained DRUNet,
deepinv's `optim_builder(iteration="HQS", prior=PnP(DRUNet), data_fidelity=L2(), params_algo=get_DPIR_params(..))`.
deepinv is not part of the reference tree, so this restates deepinv v0.2.0's documented behaviour; parity with deepinv
itself is UNPINNED. The pinned truth is the float64 restatement in tests/drunet_ref.py (pnp_ref).

Schedule. get_DPIR_params(s) for the image noise level s (the reference passes noise_level / 255 and replaces 0 by 1e-5):
max_iter = 8, sigma_k = float32(logspace(log10(49 / 255), log10(s), 8)), stepsize_k = (sigma_k / max(0.01, s))^2 / 0.23,
lambda = 1.

Iteration. x_0 = A_adjoint(y); for k = 0 .. 7: u = prox_l2(x_k, y, gamma = stepsize_k), x_{k+1} = DRUNet(u, sigma_k).
With early_stop (the reference's factory passes True) and k > 1 it stops once ||x_k - x_{k+1}|| / (||x_{k+1}|| + 1e-6)
< 1e-5 (whole-tensor norms). `iterations_run` holds the count of the last forward.

prox_l2(x, y, gamma) = argmin_u gamma / 2 ||A u - y||^2 + 1 / 2 ||u - x||^2 solves (A^T A + I / gamma) u = A^T y + x / gamma
by conjugate gradients from zero with deepinv's recurrences (alpha = rs / (p . Ap), stop when sqrt(rs_new) < tol,
p = r + p rs_new / rs), cg_max_iter = 50 and cg_tol = 1e-3 (the LinearPhysics defaults). The stopping test reads one
scalar on the host per CG iteration, as deepinv's does. The inner products are torch reductions; A and A_adjoint are the
physics' own HIP kernels, the denoiser is models/drunet.py. Any physics with A and A_adjoint qualifies.
"""
import numpy as np
import torch
from torch.nn import Module

import _native as N


def get_DPIR_params(noise_level_img):
    """(sigma_denoiser list, stepsize list, max_iter) of deepinv.optim.dpir.get_DPIR_params."""
    max_iter = 8
    s1, s2 = 49.0 / 255.0, float(noise_level_img)
    sigma = np.logspace(np.log10(s1), np.log10(s2), max_iter).astype(np.float32)
    stepsize = (sigma / max(0.01, noise_level_img)) ** 2
    lamb = 1 / 0.23
    return [float(v) for v in sigma], [float(v) for v in stepsize * lamb], max_iter


def conjugate_gradient(op, b, max_iter=50, tol=1e-3):
    """deepinv.optim.utils.conjugate_gradient: op(x) = b from x = 0 for a symmetric positive definite `op`."""
    dot = lambda u, v: (u * v).flatten().sum()          # noqa: E731
    x = torch.zeros_like(b)
    r = b.clone()
    p = r
    rs = dot(r, r)
    for _ in range(int(max_iter)):
        Ap = op(p.contiguous())
        alpha = rs / dot(p, Ap)
        x = x + p * alpha
        r = r + Ap * (-alpha)
        rs_new = dot(r, r)
        if float(rs_new.sqrt()) < tol:
            break
        p = r + p * (rs_new / rs)
        rs = rs_new
    return x


class PnPModel(Module):
    """The reference's PnPModel(physics, noise_level_img, early_stop) with the denoiser handed in (a models.drunet.DRUNet,
    or any callable (x, sigma) -> x). No parameters of its own: its state dict is empty, the denoiser's weights come from
    the file the user names."""

    def __init__(self, physics, noise_level_img, denoiser, early_stop=False, cg_max_iter=50, cg_tol=1e-3):
        super().__init__()
        if noise_level_img == 0:
            noise_level_img = 1e-5
        self.physics = physics
        self.sigma_denoiser, self.stepsize, self.max_iter = get_DPIR_params(noise_level_img)
        self._denoiser = (denoiser,)                 # in a tuple: not a submodule, so the state dict stays empty
        self.early_stop, self.cg_max_iter, self.cg_tol = bool(early_stop), int(cg_max_iter), float(cg_tol)
        self.iterations_run = 0

    @property
    def denoiser(self):
        return self._denoiser[0]

    def prox_l2(self, x, y, gamma):
        physics = self.physics
        b = physics.A_adjoint(y).contiguous() + x / gamma
        op = lambda v: physics.A_adjoint(physics.A(v).contiguous()).contiguous() + v / gamma      # noqa: E731
        return conjugate_gradient(op, b, self.cg_max_iter, self.cg_tol)

    @torch.no_grad()
    def forward(self, y):
        N.check_tensor(y.contiguous() if isinstance(y, torch.Tensor) else y, "y")
        y = y.contiguous()
        x = self.physics.A_adjoint(y).contiguous()
        self.iterations_run = 0
        for k in range(self.max_iter):
            x_prev = x
            u = self.prox_l2(x, y, self.stepsize[k])
            x = self.denoiser(u.contiguous(), self.sigma_denoiser[k])
            self.iterations_run = k + 1
            if self.early_stop and k > 1:
                crit = torch.linalg.vector_norm(x_prev - x) / (torch.linalg.vector_norm(x) + 1e-6)
                if float(crit) < 1e-5:
                    break
        return x
