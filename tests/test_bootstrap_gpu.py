"""GPU: the equivariant bootstrap's kernels (sei_boot_scale_fwd, sei_boot_luma_diff, sei_boot_pullback_accum), the host
class around them (bootstrap.EquivariantBootstrap) and test.py --bootstrap, against tests/bootstrap_ref.py.

Bars: tests/streaming_ref.py's (`same_bits`; `hold32`: within max(5e-6, 3 * ref32) of float64, ref32 the deviation of
the same torch chain in float32).

Measured on an MI355X (the largest over the cases of each row; deviation and ref32 relative to max |ref64|):

  quantity                                               ref32     bar       HIP deviation
  scale_fwd 3x8x8 B=1, 3x48x48 B=4                       7.6e-6    2.3e-5    7.6e-6, and the bits of sei_scale_resample_fwd
  scale_fwd 3x5x9 B=3, 1x17x24 B=2, 3x40x32 B=8, 3x1x7   5.4e-6    1.6e-5    5.4e-6
  luma_diff d                                            --        bits      the bits of torch's float32 chain on the CPU
  luma_diff out, (1,1x1) (3,5x9) (4,48x48) (2,200x190)   5.5e-8    5.0e-6    5.5e-8
  pullback_accum msq, the five shapes                    2.5e-6    7.4e-6    2.5e-6
  EquivariantBootstrap mse (N = 8, 3x40x32)              9.2e-6    2.7e-5    9.1e-6
  EquivariantBootstrap rmse map                          6.0e-4    1.8e-3    6.0e-4
  closed form, mean mse against 1.7242e-4                --        5 standard errors    1.7326e-4: 0.61 of one

(ref32 above 5e-6 in the gathers is the float32 sampling position; the kernels compute the same positions, hence the same
deviation. ref32 of the whole estimate is larger: a float32 value next to a rounding boundary (k + 0.5) / 255 quantises
to the other side than float64's, in the float32 torch chain as in the kernels.)
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _native as N
import bootstrap_ref as R
import streaming_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SPECIAL_CENTRES = ((-1.0, -1.0), (0.0, 0.0), (1.0, 1.0), (1.0, -1.0), (-1.0, 0.0))


def draws(B, seed):
    """Both rates in turn (starting with either), the centres -1, 0, 1 first and random ones after them."""
    gen = torch.Generator().manual_seed(seed)
    rate = torch.tensor([(0.75, 0.5)[(r + seed) % 2] for r in range(B)])
    center = 2 * torch.rand((B, 2), generator=gen) - 1
    for r in range(min(B, 3 + seed % 3)):
        center[r] = torch.tensor(SPECIAL_CENTRES[(r + seed) % len(SPECIAL_CENTRES)])
    return rate, center


def scale_fwd(x, rate, center):
    """sei_boot_scale_fwd on CPU inputs -> (B, C, H, W) on the CPU; the source is NaN-tailed, the output guarded."""
    C, H, W = x.shape
    B = rate.numel()
    got = S.Guarded((B, C, H, W))
    xd, rd, cd = S.nan_tailed(x), S.nan_tailed(rate), S.nan_tailed(center)
    N.call("sei_boot_scale_fwd", xd.data_ptr(), got.ptr(), rd.data_ptr(), cd.data_ptr(), B, C, H, W)
    torch.cuda.synchronize()
    assert got.intact()
    return got.view.cpu()


@pytest.mark.parametrize("C,H,W,B", [(3, 8, 8, 1), (3, 48, 48, 4)])
def test_scale_fwd_square_is_scale_resample_fwd(C, H, W, B):
    rate, center = draws(B, H)
    x = torch.rand((C, H, W), generator=torch.Generator().manual_seed(H))
    got = scale_fwd(x, rate, center)
    want = torch.empty((B, C, H, W), device="cuda")
    xb, rd, cd = x.cuda()[None].expand(B, C, H, W).contiguous(), rate.cuda(), center.cuda()
    N.call("sei_scale_resample_fwd", xb.data_ptr(), want.data_ptr(), rd.data_ptr(), cd.data_ptr(), B, C, H, W, H, W)
    assert S.same_bits(got, want)
    S.hold32(f"scale_fwd {C}x{H}x{W} B={B}", got, R.zoom_out(x, rate, center), R.zoom_out(x, rate, center, torch.float32))


@pytest.mark.parametrize("C,H,W,B", [(3, 5, 9, 3), (1, 17, 24, 2), (3, 40, 32, 8), (3, 1, 7, 2)])
def test_scale_fwd_not_square_against_float64_grid_sample(C, H, W, B):
    rate, center = draws(B, H + W)
    x = torch.rand((C, H, W), generator=torch.Generator().manual_seed(H * W))
    got = scale_fwd(x, rate, center)
    S.hold32(f"scale_fwd {C}x{H}x{W} B={B}", got, R.zoom_out(x, rate, center), R.zoom_out(x, rate, center, torch.float32))


def special_values():
    """float32((k + 0.5) / 255) for k = 0 .. 254 with both float32 neighbours of each, values below 0 and above 1, the ends."""
    ties = ((torch.arange(255, dtype=torch.float64) + 0.5) / 255).float()
    return torch.cat([ties, torch.nextafter(ties, torch.tensor(2.0)), torch.nextafter(ties, torch.tensor(-1.0)),
                      torch.tensor([-0.3, -1e-3, -1e-9, 0.0, 1.0, 1.0 + 1e-3, 1.7, 300.0 / 255])])


def image_pairs(batch, npix, seed):
    """a, b (batch, 3, npix) in [-0.1, 1.1]; the special values lead a and end b (as many as fit)."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.rand((batch, 3, npix), generator=gen) * 1.2 - 0.1
    b = (a + 0.05 * torch.randn((batch, 3, npix), generator=gen)).contiguous()
    sp = special_values()
    k = min(sp.numel(), a.numel())
    a.view(-1)[:k] = sp[:k]
    b.view(-1)[b.numel() - k:] = sp[:k]
    return a, b


def luma_diff(a, b, lead=0):
    """sei_boot_luma_diff on CPU inputs -> (d (batch, npix), out (batch,)) on the CPU; `lead` floats of NaN in front of the
    inputs move them off the 16-byte grid."""
    batch, _, npix = a.shape
    d, out = S.Guarded((batch, npix)), S.Guarded((batch,))
    floats = N.lib().sei_boot_luma_diff_work_floats(batch, npix)
    assert floats > 0
    work = S.Guarded((floats,))
    ad, bd = S.nan_framed(a, lead), S.nan_framed(b, lead)
    N.call("sei_boot_luma_diff", ad.data_ptr(), bd.data_ptr(), batch, npix, d.ptr(), out.ptr(), work.ptr())
    torch.cuda.synchronize()
    assert d.intact() and out.intact() and work.intact()
    return d.view.cpu(), out.view.cpu()


def ref_diff(a, b, dtype=torch.float64):
    """The reference's d for planar (batch, 3, npix) images -> (batch, npix)."""
    return R.luma_diff(a[:, :, None], b[:, :, None], dtype)[:, 0]


def test_luma_diff_bits_on_every_rounding_boundary():
    a, b = image_pairs(2, 17 * 23, seed=1)
    assert a.numel() > 2 * special_values().numel()
    d, _ = luma_diff(a, b, lead=1)
    assert S.same_bits(d, ref_diff(a, b, torch.float32))
    # the boundaries are live in this input: torch's chain sends the ties to even, their neighbours to either side
    q = R.quantize(special_values()[:255 * 3]) * 255
    assert len(set(q[:255].tolist())) >= 128 and bool((q[255:510] >= q[510:765]).all()) and bool((q[255:510] > q[510:765]).any())


@pytest.mark.parametrize("batch,H,W", [(1, 1, 1), (3, 5, 9), (4, 48, 48), (2, 200, 190)])
def test_luma_diff_sums_against_float64(batch, H, W):
    a, b = image_pairs(batch, H * W, seed=H)
    d, out = luma_diff(a, b, lead=H % 2)
    want32 = ref_diff(a, b, torch.float32)
    assert S.same_bits(d, want32)
    d64 = ref_diff(a, b)
    S.hold32(f"luma_diff out {batch}x{H}x{W}", out, (d64 * d64).sum(-1), (want32 * want32).sum(-1))


def test_luma_diff_sum_does_not_depend_on_the_batch():
    a, b = image_pairs(4, 47 * 45, seed=5)                # 3 * npix is odd: the images of a batch are 4-byte aligned only
    _, together = luma_diff(a, b)
    for i in range(4):
        _, alone = luma_diff(a[i:i + 1], b[i:i + 1], lead=i % 2)
        assert S.same_bits(alone, together[i:i + 1]), i


def pullback(d, rate, center, msq=None, accumulate=0):
    B, H, W = d.shape
    msq = msq or S.Guarded((H, W))
    dd, rd, cd = S.nan_tailed(d), S.nan_tailed(rate), S.nan_tailed(center)
    N.call("sei_boot_pullback_accum", dd.data_ptr(), rd.data_ptr(), cd.data_ptr(), B, H, W, msq.ptr(), accumulate)
    torch.cuda.synchronize()
    assert msq.intact()
    return msq


def pullback_ref(d, rate, center, dtype):
    back = R.pull_back(d, rate, center, dtype)
    return (back * back).sum(0)


@pytest.mark.parametrize("B,H,W", [(1, 8, 8), (3, 5, 9), (4, 48, 48), (2, 1, 7), (8, 40, 32)])
def test_pullback_accum_against_float64(B, H, W):
    rate, center = draws(B, B + H)
    d = 0.02 * torch.randn((B, H, W), generator=torch.Generator().manual_seed(W))
    got = pullback(d, rate, center).view.cpu()           # (accumulate = 0 over a buffer prefilled with the sentinel)
    S.hold32(f"pullback_accum {B}x{H}x{W}", got, pullback_ref(d, rate, center, torch.float64),
             pullback_ref(d, rate, center, torch.float32))


def test_pullback_accum_in_two_chunks_is_one_call():
    B, H, W = 8, 40, 32
    rate, center = draws(B, 2)
    d = 0.02 * torch.randn((B, H, W), generator=torch.Generator().manual_seed(3))
    whole = pullback(d, rate, center).view.cpu()
    parts = pullback(d[:3], rate[:3], center[:3])
    parts = pullback(d[3:].contiguous(), rate[3:].contiguous(), center[3:].contiguous(), msq=parts, accumulate=1)
    assert S.same_bits(parts.view.cpu(), whole)


# ------------------------------------------------------------------------------------------------ the host class
def blur_physics(sigma=5 / 255):
    import physics
    op = physics.BlurV2(kernel=physics.get_kernel("Gaussian_R2")[None, None].cuda())
    op.noise_model = physics.GaussianNoise(sigma=sigma)
    return op, physics.get_kernel("Gaussian_R2").double()


@pytest.fixture(scope="module")
def injected():
    """One estimate with every draw injected, N = 8 on 3 x 40 x 32 under BlurV2(Gaussian_R2) with the identity as model:
    the inputs, the float64 reference, and the same chain in float32."""
    n, H, W = 8, 40, 32
    gen = torch.Generator().manual_seed(11)
    x_hat = torch.rand((3, H, W), generator=gen) * 0.9 + 0.05
    noise = torch.randn((n, 3, H, W), generator=gen)
    rate, center = draws(n, 4)
    op, kernel = blur_physics()
    A = lambda v: R.circular_blur(v, kernel.to(v.dtype))
    r64 = R.bootstrap(x_hat, rate, center, noise, A, 5 / 255)
    r32 = R.bootstrap(x_hat, rate, center, noise, A, 5 / 255, dtype=torch.float32)
    return {"x_hat": x_hat, "noise": noise, "rate": rate, "center": center, "op": op, "r64": r64, "r32": r32, "n": n}


def run_injected(case, batch):
    from bootstrap import EquivariantBootstrap
    boot = EquivariantBootstrap(case["op"], lambda v: v, samples=case["n"], batch=batch)
    y = torch.zeros((3, 40, 32), device="cuda")          # (not read: x_hat is given and the model is the identity)
    out = boot(y, x_hat=case["x_hat"].cuda(), params=(case["rate"].cuda(), case["center"].cuda().view(-1, 1, 1, 2)),
               noise=case["noise"].cuda())
    torch.cuda.synchronize()
    return out


def test_bootstrap_with_injected_draws_against_the_reference(injected):
    """hold32 on the whole estimate. ref32 is larger here than for the kernels alone: a float32 a or b next to a rounding
    boundary (k + 0.5) / 255 quantises to the other side than float64's in the float32 torch chain too."""
    out, r64, r32, n = run_injected(injected, 8), injected["r64"], injected["r32"], injected["n"]
    assert out["mse"].shape == (n,) and out["rmse_map"].shape == (40, 32)
    S.hold32("bootstrap mse", out["mse"], r64["mse"], r32["mse"])
    S.hold32("bootstrap rmse map", out["rmse_map"], r64["rmse"], r32["rmse"])
    # the summary is the reference's arithmetic on the mse the kernels returned
    est, q90 = R.summarise(out["mse"].cpu())
    assert out["est_psnr"] == pytest.approx(est, abs=1e-9) and out["est_psnr_q90"] == pytest.approx(q90, abs=1e-9)
    assert out["est_psnr_q90"] <= out["est_psnr"]
    assert abs(out["est_psnr"] - r64["est_psnr"]) < 0.05


def test_bootstrap_chunking_does_not_change_the_bits(injected):
    two, eight = run_injected(injected, 2), run_injected(injected, 8)
    assert S.same_bits(two["mse"], eight["mse"]) and S.same_bits(two["rmse_map"], eight["rmse_map"])
    assert (two["est_psnr"], two["est_psnr_q90"]) == (eight["est_psnr"], eight["est_psnr_q90"])
    three = run_injected(injected, 3)                     # a last chunk that is not full
    assert S.same_bits(three["mse"], eight["mse"]) and S.same_bits(three["rmse_map"], eight["rmse_map"])


def test_bootstrap_closed_form_of_a_constant_image():
    """x_hat = 0.4, noise level 5, identity model: a = 0.4 = 102 / 255 for every replica, b = 0.4 + sigma n, so
    d = Y(102 / 255 - q(b)) and E d^2 = ((5^2 + 1 / 12) / 255^2) (0.299^2 + 0.587^2 + 0.114^2) = 1.7242e-4 (the variance of
    a Gaussian of 5 levels rounded to whole levels, the channels independent). The mean over N H W pixel-replicas of a
    chi-square-like d^2 has the standard error value * sqrt(2 / (N H W)); 5 of them is the bar."""
    from bootstrap import EquivariantBootstrap
    n, H, W = 16, 48, 40
    op, _ = blur_physics(5 / 255)
    torch.manual_seed(0)
    boot = EquivariantBootstrap(op, lambda v: v, samples=n, batch=8)
    x_hat = torch.full((3, H, W), 0.4, device="cuda")
    out = boot(torch.zeros_like(x_hat), x_hat=x_hat)
    value = (25 + 1 / 12) / 255 ** 2 * (0.299 ** 2 + 0.587 ** 2 + 0.114 ** 2)
    se = value * math.sqrt(2 / (n * H * W))
    mean = float(out["mse"].double().mean())
    print(f"closed form: mean mse {mean:.5e}, value {value:.5e}, {abs(mean - value) / se:.2f} standard errors")
    assert abs(mean - value) <= 5 * se
    assert out["est_psnr"] == pytest.approx(10 * math.log10(1 / mean), abs=1e-6)


def small_unet_args(*more):
    from settings import DefaultArgParser
    return DefaultArgParser().parse_args(["--device", "cuda", "--task", "deblurring", "--kernel", "Gaussian_R2",
                                          "--ProposedModel__architecture", "Convolutional",
                                          "--ConvolutionalModel__hidden_channels", "8", "--ConvolutionalModel__scales", "3",
                                          *more])


def test_bootstrap_around_the_small_unet():
    from bootstrap import EquivariantBootstrap
    from models import get_model
    from physics import get_physics
    args = small_unet_args()
    torch.manual_seed(0)
    op = get_physics(args, device="cuda")
    model = get_model(args=args, physics=op, device="cuda").to("cuda").eval()
    y = op(torch.rand((1, 3, 48, 40), device="cuda"))
    out = EquivariantBootstrap(op, model, samples=5, batch=2)(y)
    assert out["mse"].shape == (5,) and out["rmse_map"].shape == (48, 40)
    assert bool(torch.isfinite(out["mse"]).all()) and bool(torch.isfinite(out["rmse_map"]).all())
    assert bool((out["mse"] > 0).all()) and math.isfinite(out["est_psnr"]) and out["est_psnr_q90"] <= out["est_psnr"]


# ------------------------------------------------------------------------------------------------ test.py
from test_eval_metrics_gpu import COMMON, run_test_py, summary  # noqa: E402


def boot_lines(lines):
    return [(float(ln.split("EST_PSNR:")[1].split(",")[0]), float(ln.split("EST_PSNR_Q90:")[1]))
            for ln in lines if ln.startswith("BOOTSTRAP_")]


def test_test_py_bootstrap_on_the_synthetic_dataset(tmp_path):
    from PIL import Image
    out = tmp_path / "eval"
    flags = ["--task", "deblurring", "--print_all_metrics", "--bootstrap_maps", "--save_images", "--out_dir", str(out)]
    lines = run_test_py(*flags, "--bootstrap", "4", "--bootstrap_batch", "2")
    per = boot_lines(lines)
    assert len(per) == 2 and all(math.isfinite(e) and q <= e for e, q in per)
    assert summary(lines, "EST_N") == 2 and math.isfinite(summary(lines, "EST_PSNR"))
    assert math.isfinite(summary(lines, "EST_PSNR std")) and math.isfinite(summary(lines, "EST_PSNR_Q90"))
    assert abs(summary(lines, "EST_PSNR") - np.mean([e for e, _ in per])) < 0.011
    assert "N: 2" in lines and math.isfinite(summary(lines, "PSNR"))          # the ground-truth metrics stand beside it
    for i in range(2):
        w, h = Image.open(out / "estimates" / f"{i}.png").size
        rmse = np.load(out / "error_maps" / f"{i}.npy")
        assert rmse.dtype == np.float32 and rmse.shape == (h, w) and np.isfinite(rmse).all() and rmse.max() > 0
        png = np.asarray(Image.open(out / "error_maps" / f"{i}.png"))
        assert png.shape == (h, w) and png.max() == 255

    plain = run_test_py(*flags)
    assert not [ln for ln in plain if ln.startswith("EST_") or ln.startswith("BOOTSTRAP_")]
    assert "N: 2" in plain
    # the bootstrap draws under a forked generator: every line the plain run prints is there, unchanged and in order
    assert [ln for ln in lines if not (ln.startswith("EST_") or ln.startswith("BOOTSTRAP_"))] == plain
    assert len([ln for ln in plain if ln.startswith("METRICS_")]) == 2


def test_test_py_bootstrap_on_a_folder_of_measurements(tmp_path):
    from PIL import Image
    folder = tmp_path / "measurements"
    folder.mkdir()
    rng = np.random.default_rng(0)
    for name in ("a.png", "b.png"):
        Image.fromarray(rng.integers(0, 256, size=(24, 40, 3), dtype=np.uint8)).save(folder / name)
    model_flags = COMMON[COMMON.index("--kernel"):COMMON.index("--indices")]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), "--device", "cuda", "--dataset", str(folder), "--task",
                        "deblurring", *model_flags, "--bootstrap", "4", "--bootstrap_maps", "--out_dir", str(tmp_path / "o")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert "EST_N: 2" in lines and math.isfinite(summary(lines, "EST_PSNR"))
    assert not [ln for ln in lines if ln.startswith("N:")]                     # no ground truth, no PSNR
    for name in ("a", "b"):
        assert np.load(tmp_path / "o" / "error_maps" / f"{name}.npy").shape == (24, 40)
