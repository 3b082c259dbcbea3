"""The tomography-like filter (reference: src/physics/ct_like_filter.py), --task invert_a_tomography_like_filter.

`A` divides the one-sided spectrum by the ramp k + eps along H, then along W; `A_dagger` multiplies by it. Per axis
that is a real symmetric circulant matrix (physics/_circulant.py), so per image plane

    A(x) = C_H x C_W^T  (w = 1/(f+eps)),     A_dagger(y) = D_H y D_W^T  (w = f+eps),     D = C^-1

and both run as one launch of sei_circ_filter_sep (dense circular convolutions out of LDS, no FFT library).
"""
from ._base import LinearPhysics
from ._ops import CirculantFilterOp, apply_linear


class CTLikeFilter(LinearPhysics):
    def __init__(self, eps=1):
        super().__init__()
        self.eps = eps
        self._fwd = CirculantFilterOp(inverse=True, eps=eps)                  # A
        self._inv = CirculantFilterOp(inverse=False, eps=eps)                 # A_dagger
        self._axis = {(d, inv): CirculantFilterOp(inverse=inv, eps=eps, dims=(d,))
                      for d in (2, 3) for inv in (False, True)}               # filter1d

    def A(self, x):
        return apply_linear(self._fwd, x.contiguous())

    def A_adjoint(self, y):
        """A itself: the circulants are symmetric. (The reference class defines no A_adjoint and nothing on this
        task's train / test paths calls the one it inherits; the true adjoint is what this returns.)"""
        return apply_linear(self._fwd, y.contiguous())

    def A_dagger(self, y):
        """The exact inverse of A (reference :15-18), not the conjugate-gradient default of LinearPhysics."""
        return apply_linear(self._inv, y.contiguous())

    def filter1d(self, x, dim, inverse=False):
        """One axis of a (B, C, H, W) image (reference :20-39): dim 2 or 3 (or -2, -1). The other axis gets the
        identity column [1, 0, ..., 0] in the same kernel."""
        if x.dim() != 4:
            raise ValueError("filter1d: expected a (B, C, H, W) image")
        d = int(dim) % 4
        if d not in (2, 3):
            raise ValueError(f"filter1d: dim must be one of the two image axes (2 or 3), got {dim}")
        return apply_linear(self._axis[(d, bool(inverse))], x.contiguous())
