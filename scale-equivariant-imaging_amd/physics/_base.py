"""Minimal stand-ins for the deepinv classes the reference builds its physics on
(deepinv v0.2.0 `LinearPhysics`, `GaussianNoise`; not vendored in the reference, restated from their
documented behaviour -- SURVEY.md a6, 8c)."""
import torch
from torch.nn import Module

from ._ops import axpy, axpy_hetero_dev, axpy_sqrt_dev


class GaussianNoise(Module):
    """y + sigma * N(0, 1), drawn from the global torch generator of y's device."""

    def __init__(self, sigma=0.1):
        super().__init__()
        self.sigma = sigma

    def forward(self, x, noise=None, noise_sigma2=None, noise_state_pg=None):
        """noise_sigma2: a float32 device tensor whose first element stands for sigma^2 in the place of `self.sigma`
        (negative: no noise); the kernel reads it from device memory, so a captured step follows a level that moves.
        noise_state_pg: the eight-float state of losses/sure.py's SurePoissonGaussianLoss instead: the variance at a pixel
        is state[0] + state[4] x there (unit normal `noise` scaled per pixel: the Gaussian approximation of the model)."""
        if noise is None:
            noise = torch.randn_like(x)
        if noise_state_pg is not None:
            return axpy_hetero_dev(x.contiguous(), noise.contiguous(), noise_state_pg)
        if noise_sigma2 is not None:
            return axpy_sqrt_dev(x.contiguous(), noise.contiguous(), noise_sigma2)
        return axpy(x.contiguous(), noise.contiguous(), self.sigma)


class PoissonGaussianNoise(GaussianNoise):
    """gain * Poisson(max(x, 0) / gain) + sigma * N(0, 1): shot noise of `gain` image units per count plus read noise, so
    that the variance at a pixel is sigma^2 + gain * x (deepinv's PoissonGaussianNoise, restated from its documented
    behaviour). Both draws come from the global torch generator of x's device (torch's sampler: this runs where
    measurements are made, not inside the training step), the NORMAL one first: on ROCm torch.poisson reserves 20 Philox
    counters per thread, but the sampler behind it consumes about one per count below a rate of 64, so whatever the same
    generator draws next overlaps with it (measured on an MI355X at a rate of 50: a correlation of -0.069 between the
    counts and a randn_like that follows, none when it precedes; the counts' own mean and variance are right). For the
    same reason the generator is moved past the counters a Poisson draw can have used before anything else draws from it.
    `.sigma` is the Gaussian part, as test.py --r2r reads it. gain == 0 is GaussianNoise, the same draws and bits.

    Inside a loss the caller hands in what it has: `noise_state_pg` / `noise_sigma2` (estimated levels in device memory)
    go to GaussianNoise.forward; a unit normal `noise` alone is scaled per pixel to this model's own variance,
    sqrt(sigma^2 + gain x), through the same kernel (no Poisson draw: the step's draws are hoisted unit normals)."""

    def __init__(self, sigma=0.1, gain=0.0):
        super().__init__(sigma=sigma)
        if gain < 0:
            raise ValueError(f"PoissonGaussianNoise: the gain must not be negative, got {gain}")
        self.gain = gain
        self._own_state = None

    def forward(self, x, noise=None, noise_sigma2=None, noise_state_pg=None):
        if self.gain == 0 or noise_sigma2 is not None or noise_state_pg is not None:
            return super().forward(x, noise=noise, noise_sigma2=noise_sigma2, noise_state_pg=noise_state_pg)
        if noise is not None:
            if self._own_state is None or self._own_state.device != x.device:
                self._own_state = torch.tensor([self.sigma ** 2, 0, 0, 0, self.gain, 0, 0, 0], dtype=torch.float32,
                                               device=x.device)
            return super().forward(x, noise=noise, noise_state_pg=self._own_state)
        normal = torch.randn_like(x)
        counts = torch.poisson(x.clamp_min(0) / self.gain)
        if x.is_cuda:
            # below a rate of 64 a count k costs k + 1 uniform doubles, two 32-bit words each; k stays under 144 (10 standard
            # deviations past 64), so under 73 four-word counters, of which torch reserved 20: 128 more clears them
            index = x.device.index if x.device.index is not None else torch.cuda.current_device()
            generator = torch.cuda.default_generators[index]
            generator.set_offset(generator.get_offset() + 128)
        return axpy((self.gain * counts).contiguous(), normal, self.sigma)


def _conjugate_gradient(op, b, max_iter, tol):
    """deepinv.optim.utils.conjugate_gradient (v0.2.0): x from 0, stop when the squared residual falls below tol^2."""
    dot = lambda u, v: (u * v).flatten().sum()
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
        if float(rs_new) < tol ** 2:
            break
        p = r + p * (rs_new / rs)
        rs = rs_new
    return x


class LinearPhysics(Module):
    """Protocol: A, A_adjoint, __call__(x) = noise_model(A(x)), attribute noise_model."""

    def __init__(self, **kwargs):
        super().__init__()
        self.noise_model = lambda x: x

    def A(self, x):
        raise NotImplementedError

    def A_adjoint(self, y):
        raise NotImplementedError

    max_iter, tol = 50, 1e-3        # deepinv v0.2.0 LinearPhysics defaults

    def A_dagger(self, y):
        """Least-squares pseudo-inverse by conjugate gradients on the normal equations, as deepinv v0.2.0's
        LinearPhysics.A_dagger does (restated from its documented behaviour: UNPINNED; used by the `InverseFilter` model
        kind, /root/reference/src/models/__init__.py:22-28, never by the training step): with an over-complete operator
        (fewer unknowns than measurements) solve A^T A x = A^T y, otherwise A A^T u = y and return A^T u. Built on this
        operator's own A / A_adjoint (the HIP kernels); the handful of inner products are torch reductions."""
        Aty = self.A_adjoint(y)
        overcomplete = Aty.numel() < y.numel()
        if overcomplete:
            op, b = (lambda v: self.A_adjoint(self.A(v))), Aty
        else:
            op, b = (lambda v: self.A(self.A_adjoint(v))), y
        x = _conjugate_gradient(op, b, self.max_iter, self.tol)
        return x if overcomplete else self.A_adjoint(x)

    def forward(self, x):
        return self.noise_model(self.A(x))
