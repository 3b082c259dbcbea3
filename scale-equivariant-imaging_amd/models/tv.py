"""The total-variation baseline (reference: src/models/tv.py): proximal gradient descent on

    0.5 ||A x - y||^2 + lambd TV(x)

with deepinv's `optim_builder(iteration="PGD", prior=TVPrior(n_it_max), data_fidelity=L2(), ...)`. deepinv is not part of
the reference tree, so this restates deepinv v0.2.0's documented behaviour; parity with deepinv itself is UNPINNED. The
pinned truth is the float64 restatement in tests/test_tv_baseline.py.

Discrete gradient. `nabla` maps (.., H, W) to two planes, dv[i, j] = x[i+1, j] - x[i, j] for i < H - 1 else 0 and
dh[i, j] = x[i, j+1] - x[i, j] for j < W - 1 else 0 (Neumann, not wrapped); `nabla_adjoint` is its exact transpose.
Channels and batch items are independent planes; the norm is isotropic over the two directions of one pixel of one plane.

Prox. prox(z, ths) keeps a state (x2, u2) and repeats, n_it_max times, with tau = 0.01, sigma = 1 / (8 tau) = 12.5 and
rho = 1.99:

    x  = (x2 - tau * nabla_adjoint(u2) + tau * z) / (1 + tau)
    v  = u2 + sigma * nabla(2 x - x2)
    u  = v / max(|v|_2 / ths, 1)
    x2 = x2 + rho * (x - x2);   u2 = u2 + rho * (u - u2)

and returns x2. The whole loop runs in sei_tv_prox (csrc/tv_kernels.hip), several iterations per launch.

Outer loop. x_0 = A_adjoint(y); for it = 0 .. max_iter - 1: z = x - stepsize * A_adjoint(A(x) - y), x = prox(z, lambd *
stepsize); with early_stop and it > 1, stop once ||x_prev - x|| / (||x|| + 1e-6) < 1e-5 (norms over the whole tensor).
The first prox of a forward starts from x2 = z, u2 = 0; every later one continues from the state the previous one left,
which is what makes 20 inner iterations enough.

Two deliberate deviations from deepinv:
- The state is reset at the start of every `forward`. deepinv carries it over to the next image of equal shape, so its
  result depends on the order of evaluation.
- The inner loop always runs n_it_max iterations. deepinv's inner test (crit = 1e-8) needs a global norm and a host
  synchronisation per inner iteration, and at float32 it fires only once the iterate moves by about an ulp.
"""
import torch
from torch.nn import Module

import _native as N
from physics._ops import axpy


def _staged(t):
    """`t` as the kernel needs it: contiguous and on the 4-byte grid (a copy only where it is not)."""
    t = t.contiguous()
    return t if N.aligned(t, to=4) else t.clone()


def tv_prox(z, ths, state=None, iters=20, _tile=0, _k=0):
    """`iters` iterations of the primal-dual loop for prox_{ths TV}(z) on a float32 GPU tensor (.., H, W).

    `state` is (x2, u2) with u2 of shape (2,) + z.shape (vertical, then horizontal differences), or None for the cold
    start x2 = z, u2 = 0. Returns (x, state): x is a fresh tensor; the state tensors given are advanced IN PLACE and
    returned (staged copies of them where they were not contiguous). No autograd. `_tile` / `_k` pick the schedule of
    sei_tv_prox_ex for measurements and tests (0 = the default); the result does not depend on them."""
    N.check_tensor(z.contiguous() if isinstance(z, torch.Tensor) else z, "z")
    if z.dim() < 2:
        raise ValueError("tv_prox: expected an image tensor (..., H, W)")
    ths, iters = float(ths), int(iters)
    if not ths > 0 or iters < 1:
        raise ValueError(f"tv_prox: ths must be positive and iters >= 1, got {ths} and {iters}")
    z = _staged(z.detach())
    H, W = z.shape[-2:]
    planes = z.numel() // (H * W)
    if state is None:
        x2 = z.clone()
        u2 = torch.zeros((2,) + tuple(z.shape), dtype=torch.float32, device=z.device)
    else:
        x2, u2 = state
        N.check_tensor(x2.contiguous(), "state x2")
        N.check_tensor(u2.contiguous(), "state u2")
        if x2.shape != z.shape or tuple(u2.shape) != (2,) + tuple(z.shape):
            raise ValueError(f"tv_prox: state of shapes {tuple(x2.shape)}, {tuple(u2.shape)} for z of shape {tuple(z.shape)}")
        x2, u2 = _staged(x2.detach()), _staged(u2.detach())
    words = N.lib().sei_tv_prox_work_floats(planes, H, W)
    if words == 0:
        raise N.NativeLibraryError(f"sei_tv_prox refuses {planes} planes of {H} x {W}")
    work = torch.empty(words, dtype=torch.float32, device=z.device)
    if _tile or _k:
        N.call("sei_tv_prox_ex", z.data_ptr(), x2.data_ptr(), u2.data_ptr(), planes, H, W, ths, iters, int(_tile), int(_k),
               work.data_ptr())
    else:
        N.call("sei_tv_prox", z.data_ptr(), x2.data_ptr(), u2.data_ptr(), planes, H, W, ths, iters, work.data_ptr())
    return x2.clone(), (x2, u2)


class TV(Module):
    """The reference's TV(physics, lambd, stepsize=1.0, max_iter=300, n_it_max=20, early_stop=True). Any LinearPhysics:
    the iterate has the size of physics.A_adjoint(y). No parameters: its state dict is empty. `iterations_run` holds the
    number of outer iterations of the last forward."""

    def __init__(self, physics, lambd, stepsize=1.0, max_iter=300, n_it_max=20, early_stop=True):
        super().__init__()
        if lambd is None:
            raise NotImplementedError("model kind 'TV' has no default regularisation weight: give --tv_lambd")
        self.physics = physics
        self.lambd, self.stepsize = float(lambd), float(stepsize)
        self.max_iter, self.n_it_max, self.early_stop = int(max_iter), int(n_it_max), bool(early_stop)
        self.iterations_run = 0

    @torch.no_grad()
    def forward(self, y):
        N.check_tensor(y.contiguous() if isinstance(y, torch.Tensor) else y, "y")
        y = y.contiguous()
        physics = self.physics
        x = physics.A_adjoint(y).contiguous()
        state = None
        self.iterations_run = 0
        for it in range(self.max_iter):
            x_prev = x
            residual = axpy(physics.A(x).contiguous(), y, -1.0)
            z = axpy(x, physics.A_adjoint(residual).contiguous(), -self.stepsize)
            x, state = tv_prox(z, self.lambd * self.stepsize, state, self.n_it_max)
            self.iterations_run = it + 1
            if self.early_stop and it > 1:
                # one host read per outer iteration, as physics._base._conjugate_gradient does
                crit = torch.linalg.vector_norm(x_prev - x) / (torch.linalg.vector_norm(x) + 1e-6)
                if float(crit) < 1e-5:
                    break
        return x
