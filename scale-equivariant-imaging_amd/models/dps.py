"""The DPS baseline (reference: src/models/dps.py): diffusion posterior sampling, deepinv's
`DPS(model=DRUNet, data_fidelity=L2())`. deepinv is not part of the reference tree, so this restates deepinv v0.2.0's
`deepinv.sampling.DPS` as recalled; parity with deepinv itself is UNPINNED. The pinned truth is the float64 restatement in
tests/dps_ref.py. The denoiser is the DRUNet that PlugAndPlay and DiffPIR_DRUNet run, from the same --drunet_weights file:
what DPS adds is a backward pass through it, `DRUNet.forward_taped` / `DRUNet.vjp` (models/drunet.py).

Tables. betas = linspace(1e-4, 2e-2, 1000) in float32, ac = cumprod(1 - cat([0], betas)) of length 1001,
alpha(t) = ac[t + 1], so alpha(-1) = 1.

Schedule. skip = 1000 // max_iter, seq = range(0, 1000, skip), seq_next = [-1] + seq[:-1]; the pairs (i, j) of
zip(reversed(seq), reversed(seq_next)). max_iter in 1 .. 1000; anything else raises ValueError.

Start. x = randn of the IMAGE's shape, the shape of A_adjoint(y). Upstream draws randn_like(y), which only works when image
and measurement have one shape; here super-resolution runs too.

Step (i, j), with at = alpha(i), an = alpha(j):
 1. aux = x / (2 sqrt(at)) + 0.5
 2. out = D(aux, sigma = sqrt(1 - at) / sqrt(at) / 2)
 3. x0 = clamp(2 out - 1, -1, 1)
 4. r_b = A(x0 / 2 + 0.5)_b - y_b and f_b = 0.5 ||r_b||^2 per image
 5. loss = sum_b sqrt(f_b). Upstream hands the fidelity x0 in [-1, 1] and leaves the scaling of y to the caller, and the
    reference's wrapper does not scale y; this builds what it plainly intends, both sides in [0, 1].
 6. g = d loss / d x, written out: g_b = (1 / (2 sqrt(at))) s_b J_D(aux)^T [m * A^T r_b], with s_b = 1 / (2 sqrt(f_b)), taken
    as 0 when f_b = 0 (upstream would yield NaN), and m = [-1 <= 2 out - 1 <= 1]; the factor 2 of x0 and the 1 / 2 of
    x0 / 2 + 0.5 cancel. s_b is a per-image scalar and everything behind it is linear, so it is applied at the end.
 7. st = eta sqrt((1 - at / an)(1 - an) / (1 - at)), eta = 1
 8. c2 = sqrt((1 - an) - st^2)
 9. x = (sqrt(an) - c2 sqrt(at) / sqrt(1 - at)) x0 + st randn + c2 x / sqrt(1 - at) - g

A^T in step 6 is the derivative of the data term through A, as upstream's autograd takes it: the physics' `A_transpose`
where it names one (Downsampling, whose default A_adjoint is the reference's plain bicubic upsampling and no transpose),
else its A_adjoint (the blur's circular correlation is the transpose).

Result. x / 2 + 0.5. The last pair has an = 1, so st = c2 = 0 and x = x0 - g. The scalar coefficients are computed once on
the host, in float64, then rounded to float32. DPS ignores the measurement noise level: 0 is not refused.

Around the denoiser's two calls the fused path (the default) launches sei_dps_u (what A is applied to), the physics' A,
sei_dps_residual (r, f_b and s_b, the scalars written by the fold on the device), the physics' A_adjoint, sei_dps_seed (the
VJP's input) and sei_dps_step (step 9 with s_b / (2 sqrt(at)) applied to the VJP's result, in place on x, and the next
aux -- after the last pair the result -- in the same pass): no scalar crosses to the host inside the loop. `fused=False` is
the literal path, kept for comparison: torch expressions for everything but the denoiser.

Noise comes from torch's generator, as in the reference, through `draw(i, like)`: i = 0 is the start, i = k + 1 the noise
of step k. DPS makes max_iter (default 1000) denoiser evaluations per image, each a forward and a backward.
"""
import math

import numpy as np
import torch
from torch.nn import Module

import _native as N

T = 1000


def tables():
    """(betas, ac): float32 arrays of length 1000 and 1001."""
    betas = np.linspace(1e-4, 2e-2, T, dtype=np.float32)
    ac = np.cumprod(np.float32(1.0) - np.concatenate([np.zeros(1, np.float32), betas]), dtype=np.float32)
    return betas, ac


def schedule(max_iter):
    """The pairs (i, j) of the sampling loop, from noisy to clean; the last one is (0, -1)."""
    max_iter = int(max_iter)
    if not 1 <= max_iter <= T:
        raise ValueError(f"DPS: max_iter in 1 .. {T}, got {max_iter}")
    seq = list(range(0, T, T // max_iter))
    return list(zip(reversed(seq), reversed([-1] + seq[:-1])))


def coefficients(ac, i, j, eta=1.0):
    """The scalars of step (i, j), in float64 from the float32 table: sigma (the denoiser's noise level), ginv = 1 / (2
    sqrt(at)), st, c2, c0 and c1 (the factors of x0 and x in step 9) and den = 2 sqrt(an) (of the next aux)."""
    at, an = float(ac[i + 1]), float(ac[j + 1])
    st = eta * math.sqrt((1 - at / an) * (1 - an) / (1 - at))
    c2 = math.sqrt(max((1 - an) - st * st, 0.0))
    return {"at": at, "an": an, "sigma": math.sqrt(1 - at) / math.sqrt(at) / 2, "ginv": 1 / (2 * math.sqrt(at)), "st": st,
            "c2": c2, "c0": math.sqrt(an) - c2 * math.sqrt(at) / math.sqrt(1 - at), "c1": c2 / math.sqrt(1 - at),
            "den": 2 * math.sqrt(an)}


def _aligned(t):
    return t if N.aligned(t) else t.clone()


class DPS(Module):
    """deepinv's DPS around `denoiser` (a models.drunet.DRUNet, or anything with forward_taped(x, sigma) -> (out, tape) and
    vjp(tape, g) -> gx) for `physics` (A, A_adjoint). No parameters of its own: its state dict is empty, the denoiser's
    weights come from the file the user names."""

    def __init__(self, physics, denoiser, max_iter=1000, eta=1.0, fused=True):
        super().__init__()
        self.pairs = schedule(max_iter)
        self.physics = physics
        self._denoiser = (denoiser,)                 # in a tuple: not a submodule, so the state dict stays empty
        self.max_iter, self.eta, self.fused = int(max_iter), float(eta), bool(fused)
        self.betas, self.ac = tables()

    @property
    def denoiser(self):
        return self._denoiser[0]

    def alpha(self, t):
        return float(self.ac[t + 1])

    def coefficients(self, i, j):
        return coefficients(self.ac, i, j, self.eta)

    def draw(self, i, like):
        """The standard normal tensor of draw `i` (0: the start; k + 1: sampling step k). Overridable."""
        return torch.randn_like(like)

    def _transpose(self):
        return getattr(self.physics, "A_transpose", None) or self.physics.A_adjoint

    def _step_literal(self, c, out, tape, nz, x, y):
        physics = self.physics
        t = 2 * out - 1
        x0 = t.clamp(-1, 1)
        r = physics.A((x0 / 2 + 0.5).contiguous()).contiguous() - y
        f = 0.5 * (r * r).flatten(1).sum(1)
        s = torch.where(f > 0, 1 / (2 * f.sqrt()), torch.zeros_like(f))
        seed = self._transpose()(r.contiguous()).contiguous() * ((t >= -1) & (t <= 1))
        gx = self.denoiser.vjp(tape, seed.contiguous())
        g = (np.float32(c["ginv"]) * s).view(-1, 1, 1, 1) * gx
        x = ((float(np.float32(c["c0"])) * x0 + float(np.float32(c["st"])) * nz) + float(np.float32(c["c1"])) * x) - g
        return x, x / float(np.float32(c["den"])) + 0.5

    @torch.no_grad()
    def forward(self, y):
        N.check_tensor(y.contiguous() if isinstance(y, torch.Tensor) else y, "y")
        y = _aligned(y.contiguous())
        physics, denoiser = self.physics, self.denoiser
        x = _aligned(self.draw(0, physics.A_adjoint(y)).contiguous())
        B = x.shape[0]
        m, my = x.numel() // B, y.numel() // B
        xin = x / float(np.float32(2 * math.sqrt(self.alpha(self.pairs[0][0])))) + 0.5
        if self.fused:
            u, seed, r = torch.empty_like(x), torch.empty_like(x), torch.empty_like(y)
            part = torch.empty(N.lib().sei_dps_partials(B, my), dtype=torch.float32, device=x.device)
            f, s = (torch.empty(B, dtype=torch.float32, device=x.device) for _ in range(2))
        for k, (i, j) in enumerate(self.pairs):
            c = self.coefficients(i, j)
            out, tape = denoiser.forward_taped(xin, c["sigma"])
            out = out.contiguous()
            nz = self.draw(k + 1, x).contiguous()
            if not self.fused:
                x, xin = self._step_literal(c, out, tape, nz, x, y)
                continue
            out, nz = _aligned(out), _aligned(nz)
            N.call("sei_dps_u", out.data_ptr(), u.data_ptr(), B, m)
            Au = _aligned(physics.A(u).contiguous())
            N.call("sei_dps_residual", Au.data_ptr(), y.data_ptr(), r.data_ptr(), part.data_ptr(), f.data_ptr(), s.data_ptr(), B,
                   my)
            Atr = _aligned(self._transpose()(r).contiguous())
            N.call("sei_dps_seed", Atr.data_ptr(), out.data_ptr(), seed.data_ptr(), B, m)
            gx = _aligned(denoiser.vjp(tape, seed).contiguous())
            N.call("sei_dps_step", out.data_ptr(), gx.data_ptr(), nz.data_ptr(), s.data_ptr(), x.data_ptr(), xin.data_ptr(),
                   c["c0"], c["c1"], c["st"], c["ginv"], c["den"], B, m)
        return xin
