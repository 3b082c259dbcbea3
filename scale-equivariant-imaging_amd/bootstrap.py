"""Equivariant bootstrap: an estimate of a reconstruction's error from the measurement alone (build-side addition; Tachella
and Pereyra, "Equivariant bootstrapping for uncertainty quantification in imaging inverse problems", restated from the
paper -- deepinv is not here, nothing is ported and no parity with a package is claimed).

For one measurement y with x_hat = f(y) and replica r = 0 .. N-1:

  1. (rate_r, centre_r) from transforms.sample_downsampling_parameters: the draws of the EI loss, same order, same kernel;
  2. a_r = T_r x_hat, the padded zoom-out (bicubic, reflection, align_corners=True) by rate_r about centre_r. Blur,
     downsampling and the ramp filter commute with shifts, so the scale group is the one that reaches their null spaces;
  3. y_r = physics.noise_model(physics.A(a_r), noise = unit normal): Gaussian, or Poisson-Gaussian with --noise_gain;
  4. b_r = f(y_r);
  5. d_r = Y(q(a_r)) - Y(q(b_r)), q = test.py's quantize_and_clamp, Y = metrics.luma: an (H, W) plane;
  6. mse_r = sum(d_r^2) / (H W), measured in the transformed frame as the equivariant loss does: no inverse is needed.

  EST_PSNR     = 10 log10(1 / mean_r mse_r)
  EST_PSNR_Q90 = 10 log10(1 / m), m the element of index ceil(0.9 N) - 1 of the sorted mse_r
  rmse map     = sqrt(sum_r (T_r^+ d_r)^2 / N), T_r^+ the same bicubic rule sampling d_r at rate (g - c) + c.

T_r^+ is an interpolating pull-back, not the inverse of T_r: the map is a qualitative picture of where the errors sit, not
a calibrated per-pixel error bar. Whether EST_PSNR tracks the true PSNR depends on how equivariant the trained f is; no
calibration is shown here (no trained weights are part of this build).

Steps 2, 5, 6 and the map run in sei_boot_scale_fwd, sei_boot_luma_diff and sei_boot_pullback_accum (include/sei_hip.h).
Unlike sei_scale_resample_fwd, which keeps the reference's (w, h) meshgrid viewed as (h, w), they lay the grid out by rows
and columns, so an image with H != W is zoomed, not scrambled; for H == W the two are the same bits.
"""
import math

import torch

import _native as N
from transforms import sample_downsampling_parameters


class EquivariantBootstrap:
    """samples: N replicas; batch: replicas per chunk, the batch `model` and `physics.A` are called with (model kinds
    that take one image at a time need 1); rates: the table the zoom-out's rate is drawn from (ScalingTransform's). The
    padded scale transform without antialias is the only one: there is no argument to name another."""

    def __init__(self, physics, model, samples, batch=8, rates=(0.75, 0.5)):
        if int(samples) < 1 or int(batch) < 1:
            raise ValueError(f"EquivariantBootstrap: samples and batch must be positive, got {samples} and {batch}")
        if len(rates) < 1 or not all(0 < float(r) <= 1 for r in rates):
            raise ValueError(f"EquivariantBootstrap: rates must lie in (0, 1], got {rates}")
        self.physics, self.model = physics, model
        self.samples, self.batch, self.rates = int(samples), int(batch), [float(r) for r in rates]

    @staticmethod
    def _image(t, name):
        if t.dim() == 4 and t.shape[0] == 1:
            t = t[0]
        if t.dim() != 3:
            raise ValueError(f"EquivariantBootstrap: {name} must be one (C, H, W) image, got {tuple(t.shape)}")
        return N.check_tensor(t.contiguous(), name)

    def __call__(self, y, x_hat=None, params=None, noise=None):
        """y: one measurement (C, h, w) or (1, C, h, w); x_hat: f(y), evaluated here when None. params = (rate (N,),
        centre (N, 2) or (N, 1, 1, 2)) and noise (N, C, h, w) of unit normals stand in for the draws.
        -> {"mse": (N,) tensor, "est_psnr": float, "est_psnr_q90": float, "rmse_map": (H, W) tensor}."""
        n, dev = self.samples, y.device
        y = self._image(y, "y")
        with torch.no_grad():
            if x_hat is None:
                x_hat = self.model(y[None])
            x_hat = self._image(x_hat.detach(), "x_hat")
            C, H, W = x_hat.shape
            if C != 3:
                raise ValueError(f"EquivariantBootstrap: the luma needs 3 channels, got {C}")
            if params is None:
                params = sample_downsampling_parameters(n, dev, torch.float32, self.rates)
            rate = N.check_tensor(params[0].reshape(n).contiguous(), "rate")
            center = N.check_tensor(params[1].reshape(n, 2).contiguous(), "center")
            if noise is not None:
                N.check_tensor(noise, "noise")
                if noise.shape[0] != n:
                    raise ValueError(f"EquivariantBootstrap: noise for {noise.shape[0]} replicas, expected {n}")

            npix = H * W
            sums = torch.empty(n, dtype=torch.float32, device=dev)
            msq = torch.empty((H, W), dtype=torch.float32, device=dev)
            cap = min(self.batch, n)
            a_buf = torch.empty((cap, C, H, W), dtype=torch.float32, device=dev)
            d_buf = torch.empty((cap, H, W), dtype=torch.float32, device=dev)
            work = torch.empty(N.lib().sei_boot_luma_diff_work_floats(cap, npix), dtype=torch.float32, device=dev)
            for r0 in range(0, n, cap):
                b = min(cap, n - r0)
                a, rt, ct = a_buf[:b], rate[r0:r0 + b], center[r0:r0 + b]
                N.call("sei_boot_scale_fwd", x_hat.data_ptr(), a.data_ptr(), rt.data_ptr(), ct.data_ptr(), b, C, H, W)
                z = self.physics.A(a)
                nz = torch.randn_like(z) if noise is None else noise[r0:r0 + b]
                if nz.shape != z.shape:
                    raise ValueError(f"EquivariantBootstrap: noise of shape {tuple(nz.shape)} for measurements "
                                     f"{tuple(z.shape)}")
                rec = self.model(self.physics.noise_model(z, noise=nz))
                if rec.shape != a.shape:
                    raise ValueError(f"EquivariantBootstrap: the model returned {tuple(rec.shape)} for {tuple(a.shape)}")
                rec = N.check_tensor(rec.detach().contiguous(), "model output")
                N.call("sei_boot_luma_diff", a.data_ptr(), rec.data_ptr(), b, npix, d_buf.data_ptr(),
                       sums[r0:].data_ptr(), work.data_ptr())
                N.call("sei_boot_pullback_accum", d_buf.data_ptr(), rt.data_ptr(), ct.data_ptr(), b, H, W, msq.data_ptr(),
                       int(r0 > 0))
            mse = sums / npix
            rmse_map = (msq / n).sqrt()
        host = sorted(mse.double().tolist())
        mean, q90 = sum(host) / n, host[math.ceil(0.9 * n) - 1]
        psnr = lambda m: 10.0 * math.log10(1.0 / m) if m > 0 else math.inf
        return {"mse": mse, "est_psnr": psnr(mean), "est_psnr_q90": psnr(q90), "rmse_map": rmse_map}
