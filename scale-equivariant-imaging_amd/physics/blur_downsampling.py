"""The classical super-resolution degradation: y = (k * x) sampled every rate-th pixel (+ noise), the model of KAIR / DPIR /
USRNet and of deepinv's Downsampling(filter=..., factor=...). The reference has no such operator (its
src/physics/__init__.py:11 asks for "a class combining the blur and downsampling operators"); `Downsampling`, the
antialiased bicubic resize, stays the default of --task sr.

The blur part is exactly the operator --task deblurring builds from the same kernel, --blur_padding and --physics_v2
(physics/blur.py): BlurV2's circular rule, the legacy Blur's circular rule (a zero tap in front of an axis with an even
number of taps) or its replicate / reflect boundary. A(x) equals that blur's A(x)[..., phase::rate, phase::rate], and
A_adjoint(g) its A_adjoint of g zero-inserted at (phase::rate, phase::rate); neither intermediate is formed
(physics/_ops.BlurDecimateOp: sei_blur_decimate, or banded axis matrices for rank-1 kernels under replicate / reflect).
The centring against deepinv's Downsampling is not pinned here.
"""
import torch

from ._base import LinearPhysics
from ._ops import BlurDecimateOp, apply_linear


class BlurDownsampling(LinearPhysics):
    """BlurDownsampling(filter (1, 1, kv, kh), rate, padding, phase, v2). The filter is `.sr_filter` -- NOT `.filter` or
    `.kernel`: BM3D, the inverse filter and Noise2Inverse read those names as "this is a deblurring operator" and would
    deconvolve without upsampling; they keep refusing this physics as they refuse Downsampling."""

    PADDINGS = ("circular", "replicate", "reflect")

    def __init__(self, filter, rate, padding="circular", phase=0, v2=True, true_adjoint=True):
        super().__init__()
        if padding == "valid":
            raise ValueError("BlurDownsampling: padding='valid' is not supported (the image is then not rate times the "
                             f"measurement); use one of {self.PADDINGS}")
        if padding not in self.PADDINGS:
            raise ValueError(f"BlurDownsampling: padding must be one of {self.PADDINGS}, got {padding!r}")
        if filter.dim() != 4 or tuple(filter.shape[:2]) != (1, 1):
            raise ValueError(f"BlurDownsampling: expected a (1, 1, kv, kh) filter, got {tuple(filter.shape)}")
        self.rate = int(rate)
        self.phase = int(phase)
        self.padding = padding
        self.true_adjoint = True          # (kept for the Downsampling call surface: there is no other adjoint here)
        self.sr_filter = filter
        taps = filter.detach()
        if padding == "circular" and not v2:      # the legacy Blur's circular rule (physics/blur.py)
            kv, kh = filter.shape[-2:]
            taps = torch.nn.functional.pad(taps, (1 - kh % 2, 0, 1 - kv % 2, 0))
        self._op = BlurDecimateOp(taps, self.rate, padding, self.phase)

    def A(self, x):
        return apply_linear(self._op, x.contiguous())

    def A_adjoint(self, y):
        return apply_linear(self._op, y.contiguous(), transpose=True)

    A_transpose = A_adjoint
