"""The DiffPIR_DRUNet baseline (reference: src/models/diffpir.py): diffusion posterior sampling with a plug-and-play
denoiser, deepinv's `DiffPIR(model=DRUNet, data_fidelity=L2(), sigma=noise level)`. deepinv is not part of the reference
tree, so this restates deepinv v0.2.0's `deepinv.sampling.DiffPIR`; parity with deepinv itself is UNPINNED. The pinned
truth is the float64 restatement in tests/diffpir_ref.py.

The reference's wrapper reads `self.diffunet` in `forward` but never sets it on the DRUNet path, so upstream this model
kind dies with an AttributeError. This builds what the wrapper plainly intends: no padding (that branch belongs to the
diffusion U-Net), the L2 data fidelity and deepinv's defaults (max_iter = 100, zeta = 0.1, lambda_ = 7). The wrapper
hands deepinv no noise level either; the schedule here is built for the physics' own, as PlugAndPlay's is.

Tables (float32, length 1000). betas = linspace(1e-4, 2e-2, 1000), ac = cumprod(1 - betas), sa = sqrt(ac),
s1m = sqrt(1 - ac), red = s1m / sa, srec = sqrt(1 / ac).

Schedule, for sigma = physics.noise_model.sigma. sigmas[i] = red[999 - i], rhos[i] = lambda_ sigma^2 / red[i]^2,
seq = [int(v) for v in sqrt(linspace(0, 1000^2, max_iter))] with the last entry lowered by 1, nearest(v) = argmin |red - v|.

Forward. x = 2 A_adjoint(y) - 1; for i in range(len(seq)): cs = sigmas[seq[i]], t = nearest(cs), at = 1 / srec[t]^2;
at i = 0, x = (x + cs randn) / srec[999]; out = denoiser(x / (2 sqrt(at)) + 0.5, cs / 2); x0 = clamp(2 out - 1, -1, 1);
unless seq[i] == seq[-1]: u = prox_l2(x0 / 2 + 0.5, y, gamma = 1 / (2 rhos[t])) (the normal equations of models/pnp.py),
x0 = 2 u - 1, tn = nearest(sigmas[seq[i + 1]]), eps = (x - sa[t] x0) / s1m[t],
x = sa[tn] x0 + s1m[tn] (sqrt(1 - zeta) eps + sqrt(zeta) randn). The result is x0 / 2 + 0.5.

Between two denoiser calls the fused path (the default) launches: sei_cg_init with the DiffPIR prologue (the clamp chain
and the right-hand side in one pass), per conjugate-gradient iteration the physics' A and A_adjoint kernels and
sei_cg_apply / _update / _direction with the stopping test on the device (models/_cg.py), and one sei_diffpir_sample that
also writes the next denoiser input. `fused_cg=False` is the literal path, kept for comparison: models.pnp's torch
conjugate gradients with one host read per iteration, and torch expressions for everything else.

Noise comes from torch's generator, as in the reference, through `draw(i, like)`: i = 0 is the initial noise, i = k + 1
the noise of sampling step k. `cg_iterations` lists the conjugate-gradient iteration count of every prox of the last
forward. sigma = 0 makes the data step's gamma infinite and is refused.

The DiffPIR_DiffUNet baseline is `DiffPIRDiffUNet` below: the same loop around the diffusion U-Net of models/diffunet.py
(deepinv's DiffUNet(large_model=False); the user names its weights with --diffunet_weights), on the wrapper's other path
(src/models/diffpir.py:26-45): the measurement is reflect-padded at the bottom and right to multiples of 32 for deblurring
and of 16 otherwise, the loop runs on the padded measurement, and the result is cropped to rate x the unpadded extents.
The pinned truth of that path is tests/diffunet_ref.py.
"""
import numpy as np
import torch
from torch.nn import Module

import _native as N
from ._cg import FusedCG
from .pnp import conjugate_gradient

T = 1000


def tables():
    """{name: float32 array of length 1000} of deepinv's DiffPIR.get_alpha_beta."""
    betas = np.linspace(0.1 / 1000, 20 / 1000, T, dtype=np.float32)
    ac = np.cumprod(np.float32(1.0) - betas, dtype=np.float32)
    sa, s1m = np.sqrt(ac), np.sqrt(np.float32(1.0) - ac)
    return {"betas": betas, "ac": ac, "sa": sa, "s1m": s1m, "red": s1m / sa, "srec": np.sqrt(np.float32(1.0) / ac)}


def noise_schedule(sigma, lambda_, max_iter, red):
    """(rhos, sigmas, seq) of deepinv's DiffPIR.get_noise_schedule."""
    sigmas = red[::-1].copy()
    rhos = (np.float32(lambda_ * sigma ** 2) / (red * red)).astype(np.float32)
    seq = [int(v) for v in np.sqrt(np.linspace(0, T ** 2, max_iter))]
    seq[-1] = seq[-1] - 1
    return rhos, sigmas, seq


class DiffPIR(Module):
    """deepinv's DiffPIR around `denoiser` (a models.drunet.DRUNet, or any callable (x, sigma) -> x) for `physics` (A,
    A_adjoint, noise_model.sigma). No parameters of its own: its state dict is empty, the denoiser's weights come from the
    file the user names."""

    def __init__(self, physics, denoiser, max_iter=100, zeta=0.1, lambda_=7.0, cg_max_iter=50, cg_tol=1e-3, fused_cg=True):
        super().__init__()
        sigma = float(getattr(getattr(physics, "noise_model", None), "sigma", 0.0) or 0.0)
        if sigma == 0:
            raise ValueError("DiffPIR: the measurement noise level is 0, so the data step's gamma = 1 / (2 rho) is infinite; "
                             "give --noise_level above 0")
        if int(max_iter) < 2 or not 0.0 <= zeta <= 1.0:
            raise ValueError(f"DiffPIR: max_iter >= 2 and zeta in [0, 1], got {max_iter} and {zeta}")
        self.physics = physics
        self._denoiser = (denoiser,)                 # in a tuple: not a submodule, so the state dict stays empty
        self.sigma, self.max_iter, self.zeta, self.lambda_ = sigma, int(max_iter), float(zeta), float(lambda_)
        self.cg_max_iter, self.cg_tol, self.fused_cg = int(cg_max_iter), float(cg_tol), bool(fused_cg)
        self.tables = tables()
        self.rhos, self.sigmas, self.seq = noise_schedule(sigma, self.lambda_, self.max_iter, self.tables["red"])
        self.cg_iterations = []
        self._cg = None

    @property
    def denoiser(self):
        return self._denoiser[0]

    def nearest(self, value):
        return int(np.abs(self.tables["red"] - value).argmin())

    def gamma(self, t):
        return 1.0 / (2.0 * float(self.rhos[t]))

    def draw(self, i, like):
        """The standard normal tensor of draw `i` (0: the initial noise; k + 1: sampling step k). Overridable."""
        return torch.randn_like(like)

    def _solver(self, n, device):
        if self._cg is None or self._cg.n != n or self._cg.x.device != device:
            self._cg = FusedCG(n, device)
        return self._cg

    def _prox_literal(self, x0, y, gamma):
        """prox_l2 of models/pnp.py on x0 / 2 + 0.5, counting the operator calls (one per iteration run)."""
        physics, calls = self.physics, [0]
        b = physics.A_adjoint(y).contiguous() + (x0 / 2 + 0.5) / gamma

        def op(v):
            calls[0] += 1
            return physics.A_adjoint(physics.A(v).contiguous()).contiguous() + v / gamma

        u = conjugate_gradient(op, b, self.cg_max_iter, self.cg_tol)
        self.cg_iterations.append(calls[0])
        return u

    @torch.no_grad()
    def forward(self, y):
        N.check_tensor(y.contiguous() if isinstance(y, torch.Tensor) else y, "y")
        y = y.contiguous()
        physics, tb, seq, zeta = self.physics, self.tables, self.seq, self.zeta
        sa, s1m, srec = tb["sa"], tb["s1m"], tb["srec"]
        Aty = physics.A_adjoint(y).contiguous()
        x = 2 * Aty - 1
        shape = x.shape
        self.cg_iterations = []
        if self.fused_cg:
            cg = self._solver(x.numel(), x.device)
            normal = lambda p, out: physics.A_adjoint(physics.A(p.view(shape)).contiguous()).contiguous()   # noqa: E731
        x0 = xin = None
        for i in range(len(seq)):
            cs = float(self.sigmas[seq[i]])
            t = self.nearest(cs)
            at = 1.0 / float(srec[t]) ** 2
            if i == 0:
                x = (x + cs * self.draw(0, x)) / float(srec[-1])
                xin = x / (2 * float(np.sqrt(at))) + 0.5
            out = self.denoiser(xin, cs / 2).contiguous()
            if seq[i] == seq[-1]:
                x0 = (2 * out - 1).clamp(-1, 1)
                continue
            tn = self.nearest(float(self.sigmas[seq[i + 1]]))
            at_n = 1.0 / float(srec[tn]) ** 2
            nz = self.draw(i + 1, x).contiguous()
            if self.fused_cg:
                u = cg.solve(normal, out, Aty, self.gamma(t), self.cg_max_iter, self.cg_tol, prologue=True)
                self.cg_iterations.append(cg.iterations)
                if not N.aligned(nz):
                    nz = nz.clone()
                N.call("sei_diffpir_sample", u.data_ptr(), x.data_ptr(), nz.data_ptr(), xin.data_ptr(), float(sa[t]),
                       float(s1m[t]), float(sa[tn]), float(s1m[tn]), zeta, at_n, x.numel())
            else:
                x0 = (2 * out - 1).clamp(-1, 1)
                x0 = self._prox_literal(x0, y, self.gamma(t)) * 2 - 1
                eps = (x - float(sa[t]) * x0) / float(s1m[t])
                x = float(sa[tn]) * x0 + float(s1m[tn]) * (float(np.sqrt(1 - zeta)) * eps + float(np.sqrt(zeta)) * nz)
                xin = x / (2 * float(np.sqrt(at_n))) + 0.5
        return x0 / 2 + 0.5


def pad_amounts(h, w, task):
    """Rows and columns the reference's wrapper adds at the bottom and right of an h x w measurement: up to the next
    multiple of 32 for deblurring, of 16 otherwise (src/models/diffpir.py:28-35)."""
    m = 32 if task == "deblurring" else 16
    return (m - h % m) % m, (m - w % m) % m


class DiffPIRDiffUNet(DiffPIR):
    """The DiffPIR_DiffUNet baseline: the reference wrapper's `forward` on its diffusion U-Net path
    (src/models/diffpir.py:26-45) around the loop above, `denoiser` a models.diffunet.DiffUNet (or any callable
    (x, sigma) -> x that takes the padded extents). y is reflect-padded at the bottom and right (`pad_amounts`), the loop
    runs on the padded y, and the result is cropped to rate x the unpadded extents (rate = physics.rate, 1 without one).
    `task` defaults to physics.task, which physics.get_physics sets. A pad that is not smaller than its axis (reflection
    has nothing to mirror) raises ValueError. The noise level and the schedule are DiffPIR_DRUNet's."""

    def __init__(self, physics, denoiser, task=None, **kwargs):
        super().__init__(physics, denoiser, **kwargs)
        self.task = task if task is not None else getattr(physics, "task", None)
        if self.task is None:
            raise ValueError("DiffPIRDiffUNet: the padding depends on the task (deblurring: multiples of 32, otherwise 16); "
                             "give task= or a physics with a .task")

    def padded_extents(self, h, w):
        ph, pw = pad_amounts(h, w, self.task)
        if ph >= h or pw >= w:
            raise ValueError(f"DiffPIRDiffUNet: a {h} x {w} measurement would be reflect-padded by {ph} x {pw}, which is not "
                             "smaller than the axis")
        return h + ph, w + pw

    @torch.no_grad()
    def forward(self, y):
        N.check_tensor(y.contiguous() if isinstance(y, torch.Tensor) else y, "y")
        h, w = y.shape[-2:]
        hp, wp = self.padded_extents(h, w)
        if (hp, wp) != (h, w):
            y = torch.nn.functional.pad(y, (0, wp - w, 0, hp - h), mode="reflect")
        x = super().forward(y.contiguous())
        rate = int(getattr(self.physics, "rate", 1) or 1)
        return x[:, :, :rate * h, :rate * w].contiguous()
