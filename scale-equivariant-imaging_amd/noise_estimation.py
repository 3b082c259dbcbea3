"""Noise levels from the measurements alone (build-side addition; the project's own definition, in full in
include/sei_hip.h and DESIGN 4.20 -- no parity with a published estimator is claimed).

The operators of this project are blurs and antialiased downsamplings, so the diagonal Haar detail of a measurement,
t = ((a - b) - (c - d)) / 2 over a 2 x 2 quad (a b / c d), is almost pure noise with the variance of one pixel, and the
quad's mean says at which intensity. sei_noise_quad_hist counts (mean level, |t| bin) over every quad whose four pixels lie
strictly inside (0, 1) into a 64 x 256 histogram of 64-bit integers in device memory; calls accumulate, so a folder of
measurements pools into one histogram. sei_noise_fit reads the levels off it on the device: the Gaussian level `sigma` from
the pooled median of |t|, and the two levels of Var = eta + gain * signal from a weighted line through the per-level
medians. One 64-byte copy brings the result to the host.

What the numbers include and where they fail (DESIGN 4.20 has the figures): the 1/12 LSB^2 quantisation variance of 8-bit
files is part of what is reported; the gain reads low (a line fitted against a noisy abscissa); below about 256 x 256 x 3
pixels in total the two-level fit is unstable and `model_ok` is usually false: use `sigma`; texture that the operator does
not band-limit counts as noise.
"""
import math

import torch

import _native as N

LEVELS, BINS = 64, 256
FLAG_EMPTY, FLAG_POOLED_OVERFLOW, FLAG_NO_LINE, FLAG_NEGATIVE_SLOPE, FLAG_NEGATIVE_INTERCEPT = 1, 2, 4, 8, 16


class NoiseEstimator:
    """Owns the 128 KiB histogram and the eight doubles of the result on `device`."""

    def __init__(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise N.NativeLibraryError(f"NoiseEstimator on {device}: this build runs on MI355X only (HIP kernels, no CPU "
                                       "path)")
        self.hist = torch.zeros((LEVELS, BINS), dtype=torch.int64, device=device)     # (read as unsigned 64-bit counters)
        self.out = torch.zeros(8, dtype=torch.float64, device=device)

    def reset(self):
        self.hist.zero_()
        return self

    def add(self, y):
        """y: (C, H, W) or (B, C, H, W) float32 on the GPU; its quads are added to the histogram."""
        if isinstance(y, torch.Tensor) and y.dim() == 3:
            y = y[None]
        if not isinstance(y, torch.Tensor) or y.dim() != 4:
            raise ValueError(f"NoiseEstimator.add: expected a (C, H, W) or (B, C, H, W) tensor, got "
                             f"{tuple(y.shape) if isinstance(y, torch.Tensor) else type(y).__name__}")
        if y.is_cuda and y.device != self.hist.device:
            raise ValueError(f"NoiseEstimator.add: y is on {y.device}, the histogram on {self.hist.device}")
        y = N.check_tensor(y.contiguous() if y.is_cuda else y, "y")          # (a CPU tensor raises there: no CPU path)
        B, C, H, W = y.shape
        N.call("sei_noise_quad_hist", y.data_ptr(), B * C, H, W, self.hist.data_ptr(), 1)
        return self

    def estimate(self):
        """The fit on the device and one copy of 64 bytes -> dict: sigma (the Gaussian level), sigma_255 (on --noise_level's
        scale), eta and gain (Var = eta + gain * signal), levels_used, quads, flags, model_ok (the line was fitted and
        neither of its levels had to be clamped)."""
        N.call("sei_noise_fit", self.hist.data_ptr(), self.out.data_ptr())
        sigma, eta, gain, used, quads, flags = self.out.tolist()[:6]
        flags = int(flags)
        return {"sigma": sigma, "sigma_255": 255.0 * sigma, "eta": eta, "gain": gain, "levels_used": int(used),
                "quads": int(quads), "flags": flags,
                "model_ok": not flags & (FLAG_EMPTY | FLAG_NO_LINE | FLAG_NEGATIVE_SLOPE | FLAG_NEGATIVE_INTERCEPT)}


def estimate_noise(y):
    """The one-shot form: the levels of one tensor of measurements."""
    if isinstance(y, torch.Tensor) and not y.is_cuda:
        N.check_tensor(y, "y")                               # raises: no CPU path
    return NoiseEstimator(y.device).add(y).estimate()


def bootstrap_levels(est, kind):
    """(sigma, gain, notice) a physics is built from: kind "gaussian" -> (sigma, 0); "poisson_gaussian" -> (sqrt(eta),
    gain), falling back to the Gaussian level with a notice when the two-level fit did not hold."""
    if not math.isfinite(est["sigma"]):
        raise ValueError(f"--estimate_noise: no noise level could be read off the measurements (flags {est['flags']}: "
                         "no quad strictly inside (0, 1), or noise beyond the histogram)")
    if kind == "gaussian":
        return est["sigma"], 0.0, None
    if not est["model_ok"]:
        return est["sigma"], 0.0, (f"the Poisson-Gaussian fit did not hold (flags {est['flags']}, {est['levels_used']} "
                                   "levels): falling back to the Gaussian level")
    return math.sqrt(est["eta"]), est["gain"], None
