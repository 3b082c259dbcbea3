"""Blur physics (reference: src/physics/blur/__init__.py).

`BlurV2` (the default, --physics_v2) and the legacy `Blur` (--no-physics_v2) compute the same
circular convolution in the reference (FFT route :205-223 vs padded conv2d loops :38-77, agreeing to
5e-7 for odd filters); both are served here by the same LDS-tiled HIP kernel, `A_adjoint` by its transposed form.
The legacy `Blur` also takes the reference's replicate, reflect and valid boundaries (--blur_padding): banded axis
matrices through the separable resampler for rank-1 filters, sei_blur_dense_pad for the others (physics/_ops.py).
"""
import torch

from ._base import LinearPhysics
from ._bands import BLUR_PADDINGS
from ._ops import CircularBlurOp, PaddedBlurOp, apply_linear


class BlurV2(LinearPhysics):
    def __init__(self, kernel):
        super().__init__()
        self.kernel = kernel
        self.filter = self.kernel        # alias read by get_loss / demo/test.py (reference :202)
        self._op = CircularBlurOp(kernel)

    def A(self, x):
        return apply_linear(self._op, x.contiguous())

    def A_adjoint(self, y):
        return apply_linear(self._op, y.contiguous(), transpose=True)


class Blur(LinearPhysics):
    """Legacy surface: Blur(filter, padding='circular', device) with the reference's four paddings ('valid', 'circular',
    'replicate', 'reflect'; src/physics/blur/__init__.py:34-194). Filters are (1, 1, kv, kh); per-channel colour filters
    and any other padding ('zero', 'constant', ...) are rejected loudly. 'valid' measurements are smaller than the image
    by twice the padding of each axis (physics/_bands.blur_axis_offsets).

    An axis with an even number of taps reads one position further back than BlurV2 does (offset K/2 - 1, not K/2): the
    reference flips the filter and then zero-extends it to an odd length. Under 'circular' that is the circular kernel
    on the filter with a zero tap in front of such an axis."""

    def __init__(self, filter, padding="circular", device="cpu", **kwargs):
        super().__init__()
        if padding not in BLUR_PADDINGS:
            raise ValueError(f"Blur: padding must be one of {BLUR_PADDINGS}, got {padding!r}")
        if filter.dim() != 4 or tuple(filter.shape[:2]) != (1, 1):
            raise ValueError(f"Blur: expected a (1, 1, kv, kh) filter, got {tuple(filter.shape)}")
        self.padding = padding
        self.device = device
        self.filter = torch.nn.Parameter(filter, requires_grad=False).to(device)
        if padding == "circular":
            kv, kh = filter.shape[-2:]
            self._op = CircularBlurOp(torch.nn.functional.pad(filter.detach(), (1 - kh % 2, 0, 1 - kv % 2, 0)))
        else:
            self._op = PaddedBlurOp(filter, padding)

    def A(self, x):
        return apply_linear(self._op, x.contiguous())

    def A_adjoint(self, y):
        return apply_linear(self._op, y.contiguous(), transpose=True)
