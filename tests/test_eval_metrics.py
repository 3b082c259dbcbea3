"""The evaluation step's luma SSIM on the host path (metrics.ssim_fn on CPU tensors) against a float64 restatement written
here from the definition, its closed forms and argument errors; the bicubic Upsample baseline's factory; the SSIM entry
point's host-side argument checks (no GPU needed)."""
import math

import numpy as np
import pytest
import torch

import metrics

C1, C2 = 0.01 ** 2, 0.03 ** 2


def gauss11():
    i = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-((i / 1.5) ** 2) / 2)
    return g / g.sum()


def ssim_ref(a, b):
    """float64 SSIM of the luma of two (3, H, W) images: weighted moments as explicit sums over the 11 x 11 window offsets
    (every window inside the image), the SSIM formula with torchmetrics' clamped variances, the mean of the map."""
    a, b = (np.asarray(t, dtype=np.float64) for t in (a, b))
    ya = 0.299 * a[0] + 0.587 * a[1] + 0.114 * a[2]
    yb = 0.299 * b[0] + 0.587 * b[1] + 0.114 * b[2]
    h, w = ya.shape[0] - 10, ya.shape[1] - 10
    g = gauss11()
    mom = np.zeros((5, h, w))
    for i in range(11):
        for j in range(11):
            pa, pb, wt = ya[i:i + h, j:j + w], yb[i:i + h, j:j + w], g[i] * g[j]
            mom[0] += wt * pa
            mom[1] += wt * pb
            mom[2] += wt * pa * pa
            mom[3] += wt * pb * pb
            mom[4] += wt * pa * pb
    mu_a, mu_b, e_aa, e_bb, e_ab = mom
    var_a = np.maximum(e_aa - mu_a ** 2, 0.0)
    var_b = np.maximum(e_bb - mu_b ** 2, 0.0)
    cov = e_ab - mu_a * mu_b
    s = (2 * mu_a * mu_b + C1) * (2 * cov + C2) / ((mu_a ** 2 + mu_b ** 2 + C1) * (var_a + var_b + C2))
    return float(s.mean())


def image_pair(kind, shape, seed):
    """(x_hat, x) float64 in [0, 1]: "random" -- uniform noise and a noisy copy; "smooth" -- low-frequency images at a
    high level whose local variances are far below the level squared (the float32 cancellation case)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        x = torch.rand(shape, generator=g, dtype=torch.float64)
        x_hat = (x + 0.1 * torch.randn(shape, generator=g, dtype=torch.float64)).clamp(0, 1)
        return x_hat, x
    H, W = shape[-2:]
    r = torch.arange(H, dtype=torch.float64).view(H, 1)
    c = torch.arange(W, dtype=torch.float64).view(1, W)
    ph = torch.rand(shape[:-2] + (2,), generator=g, dtype=torch.float64)

    def field(p):
        return 0.8 + 0.05 * torch.sin(2 * math.pi * (r / 37.0 + p[..., 0, None, None])) \
            * torch.cos(2 * math.pi * (c / 53.0 + p[..., 1, None, None]))
    x = field(ph)
    x_hat = (field(ph + 0.02) + 0.003 * torch.randn(shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    return x_hat, x


SIZES = [(11, 11, 1), (12, 17, 1), (97, 131, 1), (64, 64, 3)]


@pytest.mark.parametrize("kind", ["random", "smooth"])
@pytest.mark.parametrize("H,W,batch", SIZES)
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.float64, 1e-9)])
def test_host_ssim_matches_float64_restatement(kind, H, W, batch, dtype, tol):
    x_hat, x = image_pair(kind, (batch, 3, H, W), seed=H * 1000 + W)
    ref = [ssim_ref(x_hat[i], x[i]) for i in range(batch)]
    got = metrics.ssim_fn(x_hat.to(dtype), x.to(dtype))
    assert got.shape == (batch,) and got.dtype == dtype
    assert max(abs(float(got[i]) - ref[i]) for i in range(batch)) < tol, (got.tolist(), ref)
    one = metrics.ssim_fn(x_hat[0].to(dtype), x[0].to(dtype))          # (3, H, W) -> a scalar
    assert one.dim() == 0 and abs(float(one) - ref[0]) < tol


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-6), (torch.float64, 1e-12)])
def test_ssim_closed_forms(dtype, tol):
    g = torch.Generator().manual_seed(3)
    x = torch.rand((3, 40, 52), generator=g, dtype=dtype)
    assert abs(float(metrics.ssim_fn(x, x)) - 1.0) < tol
    for a, b in ((0.2, 0.7), (0.9, 0.1), (0.5, 0.5)):
        ia, ib = torch.full((3, 20, 30), a, dtype=dtype), torch.full((3, 20, 30), b, dtype=dtype)
        want = (2 * a * b + C1) / (a * a + b * b + C1)
        assert abs(float(metrics.ssim_fn(ia, ib)) - want) < tol, (a, b)
    y = (x + 0.2 * torch.randn(x.shape, generator=g, dtype=dtype)).clamp(0, 1)
    assert float(metrics.ssim_fn(x, y)) == pytest.approx(float(metrics.ssim_fn(y, x)), abs=tol)
    anti = metrics.ssim_fn(x, 1 - x)                                     # anti-correlated: negative, within [-1, 1]
    assert -1.0 <= float(anti) < 0.0
    assert -1.0 <= float(metrics.ssim_fn(x, y)) <= 1.0


def test_ssim_argument_errors():
    ok = torch.rand(3, 11, 11)
    for bad in ((3, 10, 11), (3, 11, 10), (2, 3, 8, 40)):
        with pytest.raises(ValueError):
            metrics.ssim_fn(torch.rand(bad), torch.rand(bad))
    with pytest.raises(ValueError):
        metrics.ssim_fn(ok, torch.rand(3, 11, 12))
    with pytest.raises(ValueError):
        metrics.ssim_fn(torch.rand(4, 11, 11), torch.rand(4, 11, 11))      # not RGB
    metrics.ssim_fn(ok, ok)


def test_compute_metrics_ssim_flag():
    g = torch.Generator().manual_seed(5)
    x = torch.rand((3, 30, 41), generator=g)
    x_hat = (x + 0.05 * torch.randn((3, 30, 41), generator=g)).clamp(0, 1)
    psnr, ssim, lpips = metrics.compute_metrics(x, x_hat)
    assert math.isfinite(psnr) and math.isnan(ssim) and math.isnan(lpips)
    psnr2, ssim2, lpips2 = metrics.compute_metrics(x, x_hat, ssim=True)
    assert psnr2 == psnr and math.isnan(lpips2)
    assert math.isfinite(ssim2) and abs(ssim2 - ssim_ref(x.double(), x_hat.double())) < 1e-5


def _args(*flags):
    from settings import DefaultArgParser
    return DefaultArgParser().parse_args(list(flags))


def test_upsample_model_kind_is_built():
    """The bicubic baseline (reference src/models/__init__.py:137-138) builds on any device without weights; the other
    baselines still refuse."""
    from models import get_model
    model = get_model(_args("--task", "sr", "--sr_factor", "2", "--model_kind", "Upsample"), physics=None, device="cpu")
    assert list(model.parameters()) == [] and len(model.get_weights()) == 0
    model.load_weights({})
    assert model.get_backbone().factor == 2
    with pytest.raises(ValueError, match="sr_factor"):
        get_model(_args("--task", "deblurring", "--model_kind", "Upsample"), physics=None, device="cpu")
    for kind in ("DeepImagePrior", "PlugAndPlay", "BM3D", "DiffPIR_DRUNet", "DiffPIR_DiffUNet", "DPS", "TV"):
        with pytest.raises(NotImplementedError):
            get_model(_args("--task", "sr", "--sr_factor", "2", "--model_kind", kind), physics=None, device="cpu")


def test_ssim_entry_point_refuses_bad_arguments_on_the_host():
    import _native
    L = _native.lib()
    assert L.sei_ssim_luma(None, None, 1, 11, 11, None, None, None) == 10001
    assert L.sei_ssim_luma(16, 16, 0, 11, 11, 16, 16, None) == 10001           # batch < 1
    assert L.sei_ssim_luma(16, 16, 1, 10, 11, 16, 16, None) == 10001           # below the window
    assert L.sei_ssim_luma(16, 16, 1, 11, 10, 16, 16, None) == 10001
    assert L.sei_ssim_luma(16, 16, 1, 11, 11, 16, None, None) == 10001         # no workspace
    assert L.sei_ssim_luma_work_floats(1, 11, 11) == 1
    assert L.sei_ssim_luma_work_floats(2, 1356, 2040) == 2 * 32 * 43           # 64 x 32 tiles of the 2030 x 1346 map
    assert L.sei_ssim_luma_work_floats(32, 48, 48) == 32 * 2
    assert L.sei_ssim_luma_work_floats(1, 10, 40) == 0
