"""Linear image operators backed by the HIP kernels, with autograd.

Every operator here is linear, so one autograd Function serves them all: the backward of `op` is
`op` transposed (and vice versa), which also makes double-backward and `A_adjoint` trivial.
"""
import numpy as np
import torch

import _native as N
from . import _bands, _circulant


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, op, transpose, out_hw):
        ctx.op, ctx.transpose, ctx.in_hw = op, transpose, tuple(x.shape[-2:])
        return op.run(x, transpose, out_hw)

    @staticmethod
    def backward(ctx, g):
        return _Linear.apply(g.contiguous(), ctx.op, not ctx.transpose, ctx.in_hw), None, None, None


def apply_linear(op, x, transpose=False, out_hw=None):
    """op(x), or op^T(x) when transpose. `out_hw` pins the output size of a transposed resampling
    (the size of the image the forward consumed) where it is not implied by the input size."""
    return _Linear.apply(x, op, transpose, out_hw)


def _as_planes(x):
    if x.dim() < 2:
        raise ValueError("expected an image tensor (..., H, W)")
    N.check_tensor(x, "image")
    H, W = x.shape[-2:]
    planes = x.numel() // (H * W)
    return planes, H, W


class CircularBlurOp:
    """y = k (*) x, circular (reference BlurV2.A, src/physics/blur/__init__.py:205-223).
    Rank-1 kernels run the separable kernel; anything else the dense one."""

    def __init__(self, kernel2d):
        k = kernel2d.detach().to("cpu", torch.float64).reshape(kernel2d.shape[-2], kernel2d.shape[-1]).numpy()
        self.shape = k.shape
        total = k.sum()
        tv, th = k.sum(1), k.sum(0)
        sep = np.outer(tv, th) / total if total != 0 else None
        self.separable = sep is not None and np.abs(sep - k).max() <= 1e-12 * np.abs(k).max()
        if self.separable:
            self._host = (tv / total, th)
        else:
            self._host = (k,)
        self._dev = {}

    def _taps(self, device):
        if device not in self._dev:
            self._dev[device] = tuple(torch.tensor(a, dtype=torch.float32, device=device).contiguous()
                                      for a in self._host)
        return self._dev[device]

    def run(self, x, transpose, out_hw=None):
        planes, H, W = _as_planes(x)
        y = torch.empty_like(x)
        kv, kh = self.shape
        t = self._taps(x.device)
        if self.separable:
            N.call("sei_blur_sep_circ", x.data_ptr(), y.data_ptr(), t[0].data_ptr(), t[1].data_ptr(),
                   kv, kh, planes, H, W, int(transpose))
        else:
            N.call("sei_blur_dense_circ", x.data_ptr(), y.data_ptr(), t[0].data_ptr(), kv, kh, planes,
                   H, W, int(transpose))
        return y


class PaddedBlurOp:
    """y = k (*) x with a replicate, reflect or valid boundary (reference Blur: conv / conv_transpose,
    src/physics/blur/__init__.py:34-161; the axis rule is physics/_bands.blur_axis_matrix). Rank-1 kernels (the rank-1
    test of CircularBlurOp) run as two banded axis matrices through SeparableResampleOp, which transposes exactly and
    takes the rectangular `valid`; anything else runs sei_blur_dense_pad. Taps, bands and the adjoint's workspace are
    made on the first eager call per device and extent; later calls -- a capture among them -- hold launches only."""

    MODES = {"replicate": 1, "reflect": 2, "valid": 3}

    def __init__(self, kernel2d, mode):
        if mode not in self.MODES:
            raise ValueError(f"PaddedBlurOp: padding must be one of {tuple(self.MODES)}, got {mode!r}")
        k = kernel2d.detach().to("cpu", torch.float64).reshape(kernel2d.shape[-2], kernel2d.shape[-1]).numpy()
        self.mode, self.shape = mode, k.shape
        self.pad = tuple(_bands.blur_axis_offsets(K)[1] for K in k.shape)
        total = k.sum()
        tv, th = k.sum(1), k.sum(0)
        sep = np.outer(tv, th) / total if total != 0 else None
        self.separable = sep is not None and np.abs(sep - k).max() <= 1e-12 * np.abs(k).max()
        grow = 2 if mode == "valid" else 0
        if self.separable:
            tv = tv / total
            self._sep = SeparableResampleOp(lambda n: _bands.blur_axis_matrix(n, tv, mode),
                                            inverse_length=lambda n: n + grow * self.pad[0],
                                            matrix_fn_w=lambda n: _bands.blur_axis_matrix(n, th, mode),
                                            inverse_length_w=lambda n: n + grow * self.pad[1])
        else:
            self._host = k
        self._dev = {}         # device -> taps
        # (device, planes, H, W) -> the adjoint's Z canvas. Never evicted, like the bands: one padded image per distinct
        # extent, and a run sees a handful of extents. One stream at a time may use an operator's adjoint.
        self._work = {}

    def check_extent(self, H, W):
        """The image extents this boundary takes, refused by name before anything is built or launched."""
        for n, K, p in zip((H, W), self.shape, self.pad):
            if self.mode == "reflect" and p > n - 1:
                raise ValueError(f"Blur: padding='reflect' pads by {p} for a kernel of {K} taps, which an extent of {n} "
                                 f"cannot mirror (image {H}x{W}, kernel {self.shape[0]}x{self.shape[1]})")
            if self.mode == "valid" and n <= 2 * p:
                raise ValueError(f"Blur: padding='valid' needs an extent above {2 * p} for a kernel of {K} taps, got {n} "
                                 f"(image {H}x{W}, kernel {self.shape[0]}x{self.shape[1]})")

    def run(self, x, transpose, out_hw=None):
        planes, h, w = _as_planes(x)
        grow = 2 if self.mode == "valid" else 0
        # (H, W): the image's extents; the measurement-sized side is smaller by 2p in `valid`
        H, W = (h + grow * self.pad[0], w + grow * self.pad[1]) if transpose else (h, w)
        if transpose and out_hw is not None and tuple(out_hw) != (H, W):
            raise ValueError(f"Blur: the adjoint of a {out_hw[0]}x{out_hw[1]} image takes "
                             f"{out_hw[0] - grow * self.pad[0]}x{out_hw[1] - grow * self.pad[1]}, got {h}x{w}")
        self.check_extent(H, W)
        if self.separable:
            return self._sep.run(x, transpose, (H, W))
        if x.device not in self._dev:
            self._dev[x.device] = torch.tensor(self._host, dtype=torch.float32, device=x.device).contiguous()
        k = self._dev[x.device]
        kv, kh = self.shape
        mode = self.MODES[self.mode]
        ho, wo = (H, W) if transpose else (H - grow * self.pad[0], W - grow * self.pad[1])
        y = torch.empty(x.shape[:-2] + (ho, wo), dtype=x.dtype, device=x.device)
        work = None
        floats = N.lib().sei_blur_dense_pad_work_floats(planes, H, W, kv, kh, mode, int(transpose))
        if floats:
            key = (x.device, planes, H, W)
            if key not in self._work:
                self._work[key] = torch.empty(floats, dtype=torch.float32, device=x.device)
            work = self._work[key]
        N.call("sei_blur_dense_pad", x.data_ptr(), y.data_ptr(), k.data_ptr(), kv, kh, planes, H, W, mode,
               int(transpose), N.ptr(work))
        return y


class BlurDecimateOp:
    """y = (k (*) x)[..., phase::rate, phase::rate]: the blur of CircularBlurOp (mode 'circular') or PaddedBlurOp ('replicate',
    'reflect') sampled every rate-th pixel, evaluating the kept samples only (the axis rule is
    physics/_bands.blur_decimate_axis_matrix). Rank-1 kernels under replicate / reflect run as two banded axis matrices of
    step `rate` through SeparableResampleOp, which transposes exactly; everything circular and every other kernel runs
    sei_blur_decimate (`route` says which: 'bands' or 'kernel'). Taps, bands and the adjoint's workspace are made on the first
    eager call per device and extent; later calls -- a capture among them -- hold launches only. Transposing without `out_hw`
    assumes image extents (rate h, rate w)."""

    MODES = {"circular": 0, "replicate": 1, "reflect": 2}

    def __init__(self, kernel2d, rate, mode, phase=0):
        if mode == "valid":
            raise ValueError("BlurDecimateOp: padding='valid' is not part of this operator (the image is then not rate times "
                             "the measurement); use one of " + ", ".join(self.MODES))
        if mode not in self.MODES:
            raise ValueError(f"BlurDecimateOp: padding must be one of {tuple(self.MODES)}, got {mode!r}")
        rate, phase = int(rate), int(phase)
        if not 1 <= rate <= 8:
            raise ValueError(f"BlurDecimateOp: the rate must be in 1..8, got {rate}")
        if not 0 <= phase < rate:
            raise ValueError(f"BlurDecimateOp: the phase must be in [0, rate), got {phase} at rate {rate}")
        k = kernel2d.detach().to("cpu", torch.float64).reshape(kernel2d.shape[-2], kernel2d.shape[-1]).numpy()
        self.mode, self.rate, self.phase, self.shape = mode, rate, phase, k.shape
        self.pad = (0, 0) if mode == "circular" else tuple(_bands.blur_axis_offsets(K)[1] for K in k.shape)
        total = k.sum()
        tv, th = k.sum(1), k.sum(0)
        sep = np.outer(tv, th) / total if total != 0 else None
        self.separable = sep is not None and np.abs(sep - k).max() <= 1e-12 * np.abs(k).max()
        self.route = "bands" if self.separable and mode != "circular" else "kernel"
        if self.route == "bands":
            tv = tv / total
            self._sep = SeparableResampleOp(lambda n: _bands.blur_decimate_axis_matrix(n, tv, mode, rate, phase),
                                            inverse_length=lambda n: n * rate,
                                            matrix_fn_w=lambda n: _bands.blur_decimate_axis_matrix(n, th, mode, rate, phase),
                                            inverse_length_w=lambda n: n * rate)
        else:
            self._host = k
        self._dev = {}         # device -> taps
        self._work = {}        # (device, planes, H, W) -> the adjoint's Z canvas (as PaddedBlurOp: never evicted)

    def out_length(self, n):
        return (n - self.phase + self.rate - 1) // self.rate

    def check_extent(self, H, W):
        """The image extents this operator takes, refused by name before anything is built or launched."""
        for n, K, p in zip((H, W), self.shape, self.pad):
            if self.mode == "reflect" and p > n - 1:
                raise ValueError(f"BlurDownsampling: padding='reflect' pads by {p} for a kernel of {K} taps, which an extent "
                                 f"of {n} cannot mirror (image {H}x{W}, kernel {self.shape[0]}x{self.shape[1]})")
            if self.phase >= n:
                raise ValueError(f"BlurDownsampling: phase {self.phase} leaves no sample of an extent of {n} (image {H}x{W})")

    def run(self, x, transpose, out_hw=None):
        planes, h, w = _as_planes(x)
        s = self.rate
        H, W = (tuple(out_hw) if out_hw is not None else (s * h, s * w)) if transpose else (h, w)
        self.check_extent(H, W)
        ho, wo = self.out_length(H), self.out_length(W)
        if transpose and (ho, wo) != (h, w):
            raise ValueError(f"BlurDownsampling: the adjoint of a {H}x{W} image at rate {s}, phase {self.phase} takes "
                             f"{ho}x{wo}, got {h}x{w}")
        if self.route == "bands":
            return self._sep.run(x, transpose, (H, W))
        if x.device not in self._dev:
            self._dev[x.device] = torch.tensor(self._host, dtype=torch.float32, device=x.device).contiguous()
        k = self._dev[x.device]
        kv, kh = self.shape
        mode = self.MODES[self.mode]
        y = torch.empty(x.shape[:-2] + ((H, W) if transpose else (ho, wo)), dtype=x.dtype, device=x.device)
        work = None
        floats = N.lib().sei_blur_decimate_work_floats(planes, H, W, kv, kh, mode, s, int(transpose))
        if floats:
            key = (x.device, planes, H, W)
            if key not in self._work:
                self._work[key] = torch.empty(floats, dtype=torch.float32, device=x.device)
            work = self._work[key]
        N.call("sei_blur_decimate", x.data_ptr(), y.data_ptr(), k.data_ptr(), kv, kh, planes, H, W, mode, s, self.phase,
               self.phase, int(transpose), N.ptr(work))
        return y


# (n, None | inverse, eps, device) -> float32 first column; shared by every CirculantFilterOp. Never evicted: n floats
# per distinct image extent, and a run sees a handful of extents.
_CIRCULANT_COLUMNS = {}


def _circulant_column(n, inverse, eps, device):
    """The float32 first column on `device` of one filtered axis, or (inverse None) the identity column."""
    key = (n, inverse, eps, device)
    if key not in _CIRCULANT_COLUMNS:
        if inverse is None:
            c = np.zeros(n)
            c[0] = 1.0
        else:
            c = _circulant.first_column(n, inverse, eps)
        _CIRCULANT_COLUMNS[key] = torch.from_numpy(c.astype(np.float32)).to(device).contiguous()
    return _CIRCULANT_COLUMNS[key]


class CirculantFilterOp:
    """y = C_v x C_h^T with the symmetric circulants of the reference's CTLikeFilter.filter1d
    (src/physics/ct_like_filter.py:20-39; physics/_circulant.py): `inverse` picks 1/(f+eps) or f+eps, `dims` the image
    axes filtered (2 = H, 3 = W; an axis left out gets the identity column). The float32 first columns are built once
    per (extent, device) from the float64 formula and shared between operators. Symmetric, so `transpose` changes
    nothing."""

    def __init__(self, inverse, eps=1.0, dims=(2, 3)):
        self.inverse, self.eps, self.dims = bool(inverse), float(eps), tuple(dims)

    def run(self, x, transpose=False, out_hw=None):
        planes, H, W = _as_planes(x)
        cv = _circulant_column(H, self.inverse if 2 in self.dims else None, self.eps, x.device)
        ch = _circulant_column(W, self.inverse if 3 in self.dims else None, self.eps, x.device)
        y = torch.empty_like(x)
        N.call("sei_circ_filter_sep", x.data_ptr(), y.data_ptr(), cv.data_ptr(), ch.data_ptr(), planes, H, W)
        return y


class SeparableResampleOp:
    """y = Wv x Wh^T with Wv, Wh built per input size by `matrix_fn(n_in) -> dense (n_out, n_in)`.
    transpose=True applies Wv^T . Wh (the exact adjoint), taking the *output*-sized image. `matrix_fn_w` (with
    `inverse_length_w`) gives the horizontal axis a matrix of its own (PaddedBlurOp: the two tap vectors of a rank-1 kernel)."""

    def __init__(self, matrix_fn, inverse_length=None, matrix_fn_w=None, inverse_length_w=None):
        self.matrix_fn = matrix_fn
        self.inverse_length = inverse_length   # n_out -> n_in, needed to transpose without a forward
        # the horizontal axis' own matrix (and inverse length) where it differs from the vertical one
        self.matrix_fn_w = matrix_fn_w
        self.inverse_length_w = inverse_length_w if matrix_fn_w is not None else inverse_length
        self._cache = {}

    def _axis(self, n_in, device, transpose, horizontal=False):
        horizontal = horizontal and self.matrix_fn_w is not None
        key = (n_in, device, transpose) + ((True,) if horizontal else ())
        if key not in self._cache:
            dense = (self.matrix_fn_w if horizontal else self.matrix_fn)(n_in)
            if transpose:
                dense = dense.T
            w, lo, nb, step = _bands.to_band(np.ascontiguousarray(dense))
            self._cache[key] = (torch.from_numpy(w).to(device), torch.from_numpy(lo).to(device), nb, step,
                                dense.shape[0], dense.shape[1])
        return self._cache[key]

    def run(self, x, transpose, out_hw=None):
        planes, H, W = _as_planes(x)
        if transpose:
            if out_hw is not None:
                hi, wi = out_hw
            elif self.inverse_length is not None:
                hi, wi = self.inverse_length(H), self.inverse_length_w(W)
            else:
                raise RuntimeError("this resampling operator cannot be transposed without its input size")
        else:
            hi, wi = H, W
        wv, lov, nbv, sv, ho, need_h = self._axis(hi, x.device, transpose)
        wh, loh, nbh, sh, wo, need_w = self._axis(wi, x.device, transpose, horizontal=True)
        if (need_h, need_w) != (H, W):
            raise ValueError(f"resampling: image is {H}x{W} but the operator expects {need_h}x{need_w}")
        y = torch.empty(x.shape[:-2] + (ho, wo), dtype=x.dtype, device=x.device)
        N.call("sei_resample_sepband", x.data_ptr(), y.data_ptr(), planes, H, W, ho, wo,
               wv.data_ptr(), lov.data_ptr(), nbv, sv, wh.data_ptr(), loh.data_ptr(), nbh, sh)
        return y


_RESIZE_AXES = {}


def resample_to_size(x, out_h, out_w, antialias=True):
    """Bicubic resize of (.., H, W) float32 GPU images to (out_h, out_w) in one launch of the banded separable
    resampler: antialiased (the GroundTruthDataset resize, datasets/ground_truth.py) or plain
    F.interpolate(size=.., mode="bicubic", align_corners=False) (the HOMOGENEOUS_SWINIR measurement upsampling,
    src/datasets/synthetic_dataset.py:43-53). No autograd."""
    planes, H, W = _as_planes(x)
    build = _bands.aa_bicubic_matrix_to_size if antialias else _bands.plain_bicubic_matrix_to_size

    def axis(n_in, n_out):
        key = (n_in, n_out, str(x.device), bool(antialias))
        if key not in _RESIZE_AXES:
            w, lo, nb, step = _bands.to_band(build(n_in, n_out))
            _RESIZE_AXES[key] = (torch.from_numpy(w).to(x.device), torch.from_numpy(lo).to(x.device), nb, step)
        return _RESIZE_AXES[key]

    wv, lov, nbv, sv = axis(H, out_h)
    wh, loh, nbh, sh = axis(W, out_w)
    y = torch.empty(x.shape[:-2] + (out_h, out_w), dtype=x.dtype, device=x.device)
    N.call("sei_resample_sepband", x.data_ptr(), y.data_ptr(), planes, H, W, out_h, out_w,
           wv.data_ptr(), lov.data_ptr(), nbv, sv, wh.data_ptr(), loh.data_ptr(), nbh, sh)
    return y


class _Axpy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, alpha):
        N.check_tensor(a, "a")
        N.check_tensor(b, "b")
        if a.shape != b.shape:
            raise ValueError("axpy: shape mismatch")
        ctx.alpha = alpha
        # (sei_axpy reads and writes float4: an operand at a storage offset off the 16-byte grid is staged in a fresh
        # allocation first -- the same launch, the same bits)
        a, b = (t if N.aligned(t) else t.clone() for t in (a, b))
        out = torch.empty_like(a)
        N.call("sei_axpy", a.data_ptr(), b.data_ptr(), alpha, out.data_ptr(), a.numel())
        return out

    @staticmethod
    def backward(ctx, g):
        gb = g * ctx.alpha if ctx.needs_input_grad[1] else None
        return g, gb, None


def axpy(a, b, alpha):
    """a + alpha*b (measurement noise, SURE probe)."""
    return _Axpy.apply(a, b, float(alpha))


class _AxpySqrtDev(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, sigma2):
        N.check_tensor(a, "a")
        N.check_tensor(b, "b")
        N.check_tensor(sigma2, "sigma2")
        if a.shape != b.shape:
            raise ValueError("axpy: shape mismatch")
        if sigma2.numel() < 1 or sigma2.device != a.device:
            raise ValueError("axpy: sigma2 must be a float32 tensor on the device of the operands")
        ctx.sigma2 = sigma2
        a, b = (t if N.aligned(t) else t.clone() for t in (a, b))       # (as _Axpy: float4 reads and writes)
        out = torch.empty_like(a)
        N.call("sei_axpy_sqrt_dev", a.data_ptr(), b.data_ptr(), sigma2.data_ptr(), out.data_ptr(), a.numel())
        return out

    @staticmethod
    def backward(ctx, g):
        # (the level as it stands now: between forward and backward of one step nothing moves it)
        gb = g * ctx.sigma2.reshape(-1)[0].clamp_min(0).sqrt() if ctx.needs_input_grad[1] else None
        return g, gb, None


def axpy_sqrt_dev(a, b, sigma2):
    """a + sqrt(max(sigma2[0], 0)) * b with `sigma2` read from device memory by the kernel (measurement noise at a level
    that a captured step moves: losses/sure.py's `noise_state`). No gradient reaches `sigma2`."""
    return _AxpySqrtDev.apply(a, b, sigma2)


class _AxpyHeteroDev(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, state):
        N.check_tensor(a, "a")
        N.check_tensor(b, "b")
        N.check_tensor(state, "state")
        if a.shape != b.shape:
            raise ValueError("axpy: shape mismatch")
        if state.numel() != 8 or state.device != a.device:
            raise ValueError("axpy: state must hold the eight floats of the Poisson-Gaussian noise state on the device of "
                             "the operands")
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            # d out / d a = 1 + gamma b / (2 sqrt(eta + gamma a)) where the root's argument is positive: no kernel computes
            # it, and nothing here stands in for one (train.py refuses --no-ProposedLoss__stop_gradient with this model)
            raise NotImplementedError("axpy_hetero_dev: the signal-dependent noise level is not differentiated; call it on "
                                      "operands that need no gradient (EILoss(no_grad=True))")
        a, b = (t if N.aligned(t) else t.clone() for t in (a, b))       # (as _Axpy: float4 reads and writes)
        out = torch.empty_like(a)
        N.call("sei_axpy_hetero_dev", a.data_ptr(), b.data_ptr(), state.data_ptr(), out.data_ptr(), a.numel())
        return out

    @staticmethod
    def backward(ctx, g):
        return None, None, None


def axpy_hetero_dev(a, b, state):
    """a_i + sqrt(max(state[0] + state[4] a_i, 0)) * b_i with `state` read from device memory by the kernel: measurement
    noise whose variance is affine in the signal (Poisson-Gaussian), at the two levels that a captured step moves
    (losses/sure.py's SurePoissonGaussianLoss.noise_state). Operands that need no gradient only."""
    return _AxpyHeteroDev.apply(a, b, state)
