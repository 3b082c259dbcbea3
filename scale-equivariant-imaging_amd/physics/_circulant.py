"""The circulant matrices behind CTLikeFilter (reference: src/physics/ct_like_filter.py:20-39), in numpy float64.

The reference's `filter1d` along an axis of length n is irfft(rfft(x) * otf, n=n) with otf[k] = k + eps, or its
reciprocal. rfft keeps the frequencies 0 .. n//2 and irfft mirrors them back, so the full-length transfer function
is w(min(k, n - k)): real and even, hence the map is multiplication by a real SYMMETRIC circulant matrix C with

    C[i][j] = c[(i - j) mod n],   c[j] = (1/n) * sum_{k=0}^{n-1} w(min(k, n-k)) * cos(2 pi j k / n)

w(f) = 1/(f + eps) with inverse=True (the direction CTLikeFilter.A uses), w(f) = f + eps with inverse=False
(A_dagger). Holds for every n >= 1, odd or even. No GPU and no torch here: the device path takes the first column
(physics/_ops.py:CirculantFilterOp), the tests take `dense`.
"""
import numpy as np


def first_column(n, inverse, eps=1.0):
    """c[0..n) of the circulant of one `filter1d(.., inverse)` along an axis of length n (float64)."""
    n = int(n)
    if n < 1:
        raise ValueError(f"first_column: n must be >= 1, got {n}")
    k = np.arange(n)
    f = np.minimum(k, n - k).astype(np.float64)
    w = 1.0 / (f + eps) if inverse else f + eps
    # cos(2 pi j k / n) with the product reduced mod n first: the argument stays in [0, 2 pi) at any n
    phase = (np.outer(k, k) % n).astype(np.float64) * (2.0 * np.pi / n)
    return (np.cos(phase) @ w) / n


def dense(n, inverse, eps=1.0):
    """The n x n matrix C (float64): filter1d(x, inverse) along an axis is C @ x along it."""
    c = first_column(n, inverse, eps)
    i = np.arange(int(n))
    return c[(i[:, None] - i[None, :]) % int(n)]
