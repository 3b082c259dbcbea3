"""Evaluation metrics of the path: PSNR and SSIM on the luma channel, LPIPS on the RGB image (reference: src/metrics.py).

Both restate kornia.color.rgb_to_ycbcr's Y (0.299 R + 0.587 G + 0.114 B) and torchmetrics' definitions with data_range 1.
kornia and torchmetrics are absent here, so the restatements are pinned only against the oracle's own (PSNR:
oracle/torch_path.py: psnr_y) or against a float64 restatement in the tests (SSIM) -- SURVEY 8c "parity unpinned" for
this row.

- `psnr_fn`: torchmetrics.functional.peak_signal_noise_ratio = 10 log10(1 / mse). On GPU tensors the squared-error sum
  runs in sei_luma_sqerr.
- `ssim_fn`: torchmetrics.functional.structural_similarity_index_measure with its defaults: an 11-tap Gaussian window of
  sigma 1.5 per axis (exp(-(i / 1.5)^2 / 2), i = -5..5, normalised), the five weighted moments mu_x, mu_y, E[x^2], E[y^2],
  E[xy] per window, sigma_x^2 = max(E[x^2] - mu_x^2, 0) and sigma_y^2 likewise (current torchmetrics clamps both at 0),
  sigma_xy = E[xy] - mu_x mu_y, C1 = 0.01^2, C2 = 0.03^2, and
  ssim = (2 mu_x mu_y + C1)(2 sigma_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(sigma_x^2 + sigma_y^2 + C2)).
  torchmetrics reflect-pads by 5 and then crops 5 from every side of the map: the two cancel, so only the windows that
  lie inside the image count ((H-10) x (W-10) of them, H, W >= 11), and the result is the mean of that map per image.
  Unpinned beyond that restatement: the torchmetrics version the reference ran (its clamp, its float32 window taps).
  On float32 GPU tensors it runs in sei_ssim_luma; on CPU tensors as separable conv2d in the input dtype. Both compute
  the moments of the luma minus a local constant (per tile on the GPU, per image on the host): the variances and the
  covariance do not change, and the float32 cancellation of E[x^2] - mu^2 no longer scales with the image's level.
- `lpips_fn`: pyiqa.create_metric("lpips") = LPIPS v0.1 on AlexNet features, restated in `_lpips_host` and in
  include/sei_hip.h: the input scaling of lpips' normalize=True and ScalingLayer, the five ReLU outputs of torchvision's
  AlexNet `features`, per pixel the channel-normalised maps' weighted squared difference, the pixel mean per layer, the sum
  over the layers. The pretrained weights are not part of this build: an `LPIPS` object loads the two published state
  dicts from files the caller names (`LPIPS.from_files`). Parity with pyiqa's numbers is unpinned (neither the package nor
  the weights are here); the tests pin a float64 restatement with synthetic weights. On float32 GPU tensors the network
  and the distance run in sei_lpips_conv_relu / sei_lpips_maxpool / sei_lpips_layer_dist; on CPU tensors as F.conv2d /
  F.max_pool2d in the input dtype. `compute_metrics` returns NaN for it unless it is given an `LPIPS` object.
"""
import math

import torch
import torch.nn.functional as F

SSIM_TAPS = 11
_C1, _C2 = 0.01 ** 2, 0.03 ** 2


def luma(img):
    r, g, b = img[..., 0, :, :], img[..., 1, :, :], img[..., 2, :, :]
    return 0.299 * r + 0.587 * g + 0.114 * b


def psnr_fn(x_hat, x):
    """x_hat, x: (3, H, W) in [0, 1] -> scalar tensor (dB)."""
    if x_hat.is_cuda and x.is_cuda and x_hat.dtype == torch.float32 and x.dtype == torch.float32:
        import _native as N
        a, b = x_hat.contiguous(), x.contiguous()
        npix = a.shape[-2] * a.shape[-1]
        out = torch.empty(1, dtype=torch.float32, device=a.device)
        work = torch.empty(256, dtype=torch.float32, device=a.device)
        N.call("sei_luma_sqerr", a.data_ptr(), b.data_ptr(), npix, out.data_ptr(), work.data_ptr())
        err = out[0] / npix
    else:
        err = (luma(x_hat) - luma(x)).pow(2).mean()
    return 10.0 * torch.log10(1.0 / err)


def gaussian_taps(dtype=torch.float64, device="cpu"):
    """torchmetrics' _gaussian(11, 1.5), computed in float64 and rounded to `dtype`."""
    d = torch.arange(-(SSIM_TAPS // 2), SSIM_TAPS // 2 + 1, dtype=torch.float64)
    g = torch.exp(-((d / 1.5) ** 2) / 2)
    return (g / g.sum()).to(dtype=dtype, device=device)


def _ssim_host(a, b):
    """(B, 3, H, W) pairs -> (B,) in the input dtype: separable conv2d over the stacked moments."""
    ya, yb = luma(a), luma(b)                                   # (B, H, W)
    ca = ya.mean(dim=(-2, -1), keepdim=True)
    cb = yb.mean(dim=(-2, -1), keepdim=True)
    ya, yb = ya - ca, yb - cb
    B, H, W = ya.shape
    g = gaussian_taps(ya.dtype, ya.device)
    stack = torch.stack((ya, yb, ya * ya, yb * yb, ya * yb), dim=1).reshape(B * 5, 1, H, W)
    m = F.conv2d(F.conv2d(stack, g.view(1, 1, 1, -1)), g.view(1, 1, -1, 1)).reshape(B, 5, H - 10, W - 10)
    mu_a, mu_b, e_aa, e_bb, e_ab = m.unbind(1)
    var_a = (e_aa - mu_a * mu_a).clamp(min=0)
    var_b = (e_bb - mu_b * mu_b).clamp(min=0)
    cov = e_ab - mu_a * mu_b
    mu_a, mu_b = mu_a + ca, mu_b + cb
    ssim_map = (2 * mu_a * mu_b + _C1) * (2 * cov + _C2) / ((mu_a * mu_a + mu_b * mu_b + _C1) * (var_a + var_b + _C2))
    return ssim_map.mean(dim=(-2, -1))


def ssim_fn(x_hat, x):
    """x_hat, x: (3, H, W) in [0, 1] -> scalar tensor, or (B, 3, H, W) -> (B,); symmetric in its arguments.
    Float32 GPU tensors run sei_ssim_luma (no other GPU dtype: there is no eager fallback); CPU tensors the host path."""
    if x_hat.shape != x.shape:
        raise ValueError(f"ssim_fn: shapes differ: {tuple(x_hat.shape)} vs {tuple(x.shape)}")
    if x.dim() not in (3, 4) or x.shape[-3] != 3:
        raise ValueError(f"ssim_fn: expected (3, H, W) or (B, 3, H, W) RGB images, got {tuple(x.shape)}")
    H, W = x.shape[-2:]
    if H < SSIM_TAPS or W < SSIM_TAPS:
        raise ValueError(f"ssim_fn: images must be at least {SSIM_TAPS} x {SSIM_TAPS} (the Gaussian window), got {H} x {W}")
    if x_hat.device != x.device:
        raise ValueError(f"ssim_fn: operands on {x_hat.device} and {x.device}")
    batched = x.dim() == 4
    a, b = (x_hat, x) if batched else (x_hat[None], x[None])
    if not x.is_cuda:
        out = _ssim_host(a, b)
        return out if batched else out[0]
    import _native as N
    if x_hat.dtype != torch.float32 or x.dtype != torch.float32:
        raise TypeError(f"ssim_fn: GPU operands must be float32, got {x_hat.dtype} and {x.dtype}")
    a, b = a.contiguous(), b.contiguous()       # (4-byte alignment is all the kernel needs: offset views pass as they are)
    n = a.shape[0]
    out = torch.empty(n, dtype=torch.float32, device=a.device)
    work = torch.empty(N.lib().sei_ssim_luma_work_floats(n, H, W), dtype=torch.float32, device=a.device)
    N.call("sei_ssim_luma", a.data_ptr(), b.data_ptr(), n, H, W, out.data_ptr(), work.data_ptr())
    return out if batched else out[0]


def register_fn(x, x_hat):
    """Centre-crop both images to their common size (reference :33-40, torchvision CenterCrop)."""
    if x.shape[-2] != x_hat.shape[-2] or x.shape[-1] != x_hat.shape[-1]:
        hmin, wmin = min(x.shape[-2], x_hat.shape[-2]), min(x.shape[-1], x_hat.shape[-1])

        def centre(t):
            top = int(round((t.shape[-2] - hmin) / 2.0))
            left = int(round((t.shape[-1] - wmin) / 2.0))
            return t[..., top:top + hmin, left:left + wmin]
        x, x_hat = centre(x), centre(x_hat)
    return x, x_hat


# ---- LPIPS ------------------------------------------------------------------------------------------------------
LPIPS_MIN_EXTENT = 31                      # below it the second pool has fewer than 3 rows or columns
_LPIPS_SHIFT = (-0.030, -0.088, -0.188)
_LPIPS_SCALE = (0.458, 0.448, 0.450)
# torchvision AlexNet `features`: (index in the Sequential, Cin, Cout, kernel, stride, zero pad, a max-pool follows)
_ALEX = ((0, 3, 64, 11, 4, 2, True), (3, 64, 192, 5, 1, 2, True), (6, 192, 384, 3, 1, 1, False),
         (8, 384, 256, 3, 1, 1, False), (10, 256, 256, 3, 1, 1, False))


def _lpips_extents(H, W):
    """[(h, w) of the five tapped maps], [(h, w) after the two pools] for an H x W image."""
    maps, pools = [], []
    h, w = H, W
    for _, _, _, k, s, p, pool in _ALEX:
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        maps.append((h, w))
        if pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
            pools.append((h, w))
    return maps, pools


def _find_key(sd, suffix, shape, what):
    """The tensor of `sd` whose key is `suffix` or ends in '.' + suffix (a `net.` or `module.` prefix), of `shape`."""
    hits = [k for k in sd if k == suffix or k.endswith("." + suffix)]
    if not hits:
        raise ValueError(f"LPIPS {what}: key {suffix!r} of shape {tuple(shape)} is missing")
    t = sd[hits[0]]
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"LPIPS {what}: key {hits[0]!r} must have shape {tuple(shape)}, got {got}")
    return t.detach().to("cpu", torch.float32).contiguous()


class LPIPS:
    """LPIPS v0.1 (AlexNet) with weights from the two published state dicts. Holds the weights in torch's layout on the
    host (the host path, any dtype) and, on a GPU device, repacked once to the [Cout][K] rows sei_lpips_conv_relu reads."""

    def __init__(self, conv_w, conv_b, lin, device="cpu"):
        self.conv_w, self.conv_b, self.lin = list(conv_w), list(conv_b), list(lin)
        self.device = torch.device(device)
        self._packed = None
        if self.device.type == "cuda":
            if self.device.index is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
            packed = []
            for l, w in enumerate(self.conv_w):
                if l == 0:                                   # K = (ci, ky, kx), padded from 363 to 384 with zeros
                    rows = F.pad(w.reshape(w.shape[0], -1), (0, 384 - 363))
                else:                                        # K = (ky, kx, ci): a k-tile is 32 channels of one tap
                    rows = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
                packed.append(rows.contiguous().to(self.device))
            self._packed = (packed, [b.to(self.device) for b in self.conv_b],
                            [v.reshape(-1).contiguous().to(self.device) for v in self.lin])

    @classmethod
    def from_state_dicts(cls, backbone, linear, device="cpu"):
        """backbone: a torchvision AlexNet state dict (features.{0,3,6,8,10}.{weight,bias}; classifier.* and anything else
        is ignored); linear: the LPIPS v0.1 `alex` linear layers (lin{0..4}.model.1.weight, (1, C, 1, 1)). Keys match by
        suffix. A missing key or a wrong shape raises ValueError naming the key and the shape wanted."""
        conv_w, conv_b, lin = [], [], []
        for l, (idx, cin, cout, k, _, _, _) in enumerate(_ALEX):
            conv_w.append(_find_key(backbone, f"features.{idx}.weight", (cout, cin, k, k), "backbone"))
            conv_b.append(_find_key(backbone, f"features.{idx}.bias", (cout,), "backbone"))
            lin.append(_find_key(linear, f"lin{l}.model.1.weight", (1, cout, 1, 1), "linear"))
        return cls(conv_w, conv_b, lin, device)

    @classmethod
    def from_files(cls, backbone, linear, device="cpu"):
        return cls.from_state_dicts(torch.load(backbone, map_location="cpu", weights_only=True),
                                    torch.load(linear, map_location="cpu", weights_only=True), device)

    # -- host path: the readable definition --
    def _features_host(self, x):
        shift = torch.tensor(_LPIPS_SHIFT, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
        scale = torch.tensor(_LPIPS_SCALE, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
        h = ((2 * x - 1) - shift) / scale
        feats = []
        for l, (_, _, _, _, stride, pad, pool) in enumerate(_ALEX):
            h = F.relu(F.conv2d(h, self.conv_w[l].to(x.dtype), self.conv_b[l].to(x.dtype), stride=stride, padding=pad))
            feats.append(h)
            if pool:
                h = F.max_pool2d(h, 3, 2)
        return feats

    def _lpips_host(self, a, b):
        total = 0
        for l, (fa, fb) in enumerate(zip(self._features_host(a), self._features_host(b))):
            na = fa / (fa.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
            nb = fb / (fb.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
            total = total + ((na - nb).pow(2) * self.lin[l].to(a.dtype)).sum(dim=1).mean(dim=(-2, -1))
        return total

    # -- GPU path --
    def _maps_gpu(self, a, b):
        """The five maps of a's images followed by b's (b may be None), channels-last: [(n, h, w, C)], and the rest of the
        work buffer (the partial sums of the distance)."""
        import _native as N
        if self._packed is None or a.device != self.device:
            raise ValueError(f"LPIPS: built for {self.device}, operands on {a.device}")
        B, _, H, W = a.shape
        n = B if b is None else 2 * B
        pairs = (n + 1) // 2
        (hw, pools), (w, bias, _) = _lpips_extents(H, W), self._packed
        total = N.lib().sei_lpips_work_floats(pairs, H, W)
        sizes = [2 * pairs * hw[l][0] * hw[l][1] * _ALEX[l][2] for l in range(5)]
        psizes = [2 * pairs * pools[l][0] * pools[l][1] * _ALEX[l][2] for l in range(2)]
        if total != sum(sizes) + sum(psizes) + 1024 * pairs:
            raise N.NativeLibraryError(f"sei_lpips_work_floats({pairs}, {H}, {W}) = {total}: not this layer's layout")
        work = torch.empty(total, dtype=torch.float32, device=a.device)
        at, maps = 0, []
        src = None
        for l in range(5):
            out = work[at:at + sizes[l]]
            at += sizes[l]
            if l == 0:
                N.call("sei_lpips_conv_relu", a.data_ptr(), N.ptr(b), B, w[0].data_ptr(), bias[0].data_ptr(), out.data_ptr(),
                       0, n, H, W)
            else:
                N.call("sei_lpips_conv_relu", src.data_ptr(), None, n, w[l].data_ptr(), bias[l].data_ptr(), out.data_ptr(),
                       l, n, H, W)
            maps.append(out[:n * hw[l][0] * hw[l][1] * _ALEX[l][2]].view(n, hw[l][0], hw[l][1], _ALEX[l][2]))
            src = out
            if l < 2:
                src = work[at:at + psizes[l]]
                at += psizes[l]
                N.call("sei_lpips_maxpool", out.data_ptr(), src.data_ptr(), l, n, H, W)
        return maps, work[at:]

    def features(self, x):
        """x: (3, H, W) or (B, 3, H, W) in [0, 1] -> the five tapped maps (each after its ReLU) as NCHW tensors
        (B, C_l, h_l, w_l): lpips' retPerLayer view of the network."""
        x = _lpips_check(x, x, "LPIPS.features")[0]
        if not x.is_cuda:
            return self._features_host(x)
        maps, _ = self._maps_gpu(x, None)
        return [m.permute(0, 3, 1, 2) for m in maps]


def _lpips_check(x_hat, x, who):
    if x_hat.shape != x.shape:
        raise ValueError(f"{who}: shapes differ: {tuple(x_hat.shape)} vs {tuple(x.shape)}")
    if x.dim() not in (3, 4) or x.shape[-3] != 3:
        raise ValueError(f"{who}: expected (3, H, W) or (B, 3, H, W) RGB images, got {tuple(x.shape)}")
    H, W = x.shape[-2:]
    if H < LPIPS_MIN_EXTENT or W < LPIPS_MIN_EXTENT:
        raise ValueError(f"{who}: images must be at least {LPIPS_MIN_EXTENT} x {LPIPS_MIN_EXTENT} (AlexNet's second "
                         f"pool), got {H} x {W}")
    if x_hat.device != x.device:
        raise ValueError(f"{who}: operands on {x_hat.device} and {x.device}")
    if x.is_cuda and (x_hat.dtype != torch.float32 or x.dtype != torch.float32):
        raise TypeError(f"{who}: GPU operands must be float32, got {x_hat.dtype} and {x.dtype}")
    if x.dim() == 3:
        x_hat, x = x_hat[None], x[None]
    return x_hat.contiguous(), x.contiguous()


def lpips_fn(x_hat, x, net):
    """x_hat, x: (3, H, W) in [0, 1] -> scalar tensor, or (B, 3, H, W) -> (B,); symmetric in its images; `net`: an LPIPS.
    Float32 GPU tensors run the sei_lpips_* kernels (no other GPU dtype: there is no eager fallback); CPU tensors the host
    path in their dtype."""
    batched = x.dim() == 4
    a, b = _lpips_check(x_hat, x, "lpips_fn")
    if not a.is_cuda:
        out = net._lpips_host(a, b)
        return out if batched else out[0]
    import _native as N
    maps, work = net._maps_gpu(a, b)
    B, _, H, W = a.shape
    out = torch.empty(B, dtype=torch.float32, device=a.device)
    for l, m in enumerate(maps):                      # in layer order: the launches add d_l to the running sum
        N.call("sei_lpips_layer_dist", m[:B].data_ptr(), m[B:].data_ptr(), net._packed[2][l].data_ptr(), l, B, H, W,
               out.data_ptr(), int(l > 0), work.data_ptr())
    return out if batched else out[0]


def compute_metrics(x, x_hat, ssim=False, lpips=None):
    """(psnr, ssim, lpips) as the reference's compute_metrics. The SSIM is computed with ssim=True (test.py --ssim) and
    NaN otherwise; the LPIPS with lpips=an LPIPS object (test.py --lpips_backbone / --lpips_linear) and NaN otherwise."""
    x, x_hat = register_fn(x, x_hat)
    ssim_val = ssim_fn(x, x_hat).item() if ssim else math.nan
    lpips_val = lpips_fn(x, x_hat, lpips).item() if isinstance(lpips, LPIPS) else math.nan
    return psnr_fn(x, x_hat).item(), ssim_val, lpips_val
