"""GPU: the luma SSIM kernel (sei_ssim_luma, through metrics.ssim_fn) against the float64 restatement of
tests/test_eval_metrics.py, its determinism, the bicubic Upsample baseline against F.interpolate, and test.py --ssim end
to end."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metrics
from test_eval_metrics import _args, image_pair, ssim_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", ["random", "smooth"])
@pytest.mark.parametrize("H,W,batch", [(11, 11, 1), (97, 131, 1), (256, 256, 4), (48, 48, 32), (1356, 2040, 1)])
def test_ssim_kernel_matches_float64_restatement(kind, H, W, batch):
    """Per image within 1e-5 of float64 (the 11 x 11 case is one window, the 1356 x 2040 case a DIV2K validation image)."""
    x_hat, x = image_pair(kind, (batch, 3, H, W), seed=H * 1000 + W)
    x_hat, x = x_hat.float(), x.float()
    got = metrics.ssim_fn(x_hat.cuda(), x.cuda()).cpu()
    assert got.shape == (batch,)
    err = max(abs(float(got[i]) - ssim_ref(x_hat[i], x[i])) for i in range(batch))
    print(f"ssim {kind} {batch}x{H}x{W}: max |gpu - float64| = {err:.2e}")
    assert err < 1e-5


def test_ssim_kernel_at_a_storage_offset_and_against_the_host_path():
    x_hat, x = image_pair("random", (2, 3, 97, 131), seed=7)
    x_hat, x = x_hat.float(), x.float()
    buf = torch.zeros(1 + x.numel(), device="cuda")
    buf[1:] = x.flatten().cuda()
    xv = buf[1:].view(2, 3, 97, 131)                   # contiguous, 4 bytes off the 16-byte grid
    assert xv.data_ptr() % 16 != 0
    got = metrics.ssim_fn(x_hat.cuda(), xv).cpu()
    host = metrics.ssim_fn(x_hat, x)
    for i in range(2):
        assert abs(float(got[i]) - ssim_ref(x_hat[i], x[i])) < 1e-5
        assert abs(float(got[i]) - float(host[i])) < 1e-5
    assert float(metrics.ssim_fn(xv[1], xv[1])) == pytest.approx(1.0, abs=1e-6)
    with pytest.raises(TypeError):
        metrics.ssim_fn(x_hat.cuda().double(), x.cuda().double())


def test_ssim_kernel_is_deterministic_and_batch_independent():
    x_hat, x = image_pair("random", (4, 3, 256, 256), seed=11)
    a, b = x_hat.float().cuda(), x.float().cuda()
    first, second = metrics.ssim_fn(a, b), metrics.ssim_fn(a, b)
    assert torch.equal(first, second)
    singles = torch.stack([metrics.ssim_fn(a[i], b[i]) for i in range(4)])
    assert torch.equal(first, singles)


@pytest.mark.parametrize("factor", [2, 3, 4])
@pytest.mark.parametrize("hw", [(17, 24), (16, 23)])
def test_upsample_baseline_matches_bicubic_interpolation(factor, hw):
    from models import get_model
    model = get_model(_args("--task", "sr", "--sr_factor", str(factor), "--model_kind", "Upsample"), physics=None,
                      device="cuda").to("cuda").eval()
    y = torch.rand((2, 3) + hw, generator=torch.Generator().manual_seed(factor))
    with torch.no_grad():
        out = model(y.cuda())
    ref = F.interpolate(y.double(), scale_factor=factor, mode="bicubic", align_corners=False)
    assert out.shape == ref.shape
    assert float((out.cpu().double() - ref).abs().max() / ref.abs().max()) < 1e-5


COMMON = ["--device", "cuda", "--dataset", "synthetic", "--kernel", "Gaussian_R2", "--ProposedModel__architecture",
          "Convolutional", "--ConvolutionalModel__hidden_channels", "8", "--ConvolutionalModel__scales", "3", "--indices",
          "0,1"]


def run_test_py(*flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), *COMMON, *flags], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip().splitlines()


def summary(lines, key):
    return float([ln for ln in lines if ln.startswith(key + ":")][0].split()[-1])


def test_test_py_ssim(tmp_path):
    from PIL import Image
    out = tmp_path / "eval"
    lines = run_test_py("--task", "deblurring", "--ssim", "--print_all_metrics", "--save_images", "--out_dir", str(out))
    per = [float(ln.split("SSIM:")[1].split(",")[0]) for ln in lines if ln.startswith("METRICS_")]
    assert len(per) == 2 and all(math.isfinite(v) for v in per)
    assert math.isfinite(summary(lines, "SSIM std")) and abs(summary(lines, "SSIM") - np.mean(per)) < 1e-4

    def load(p):                                   # the 8-bit images the metrics saw, exactly
        a = np.asarray(Image.open(p), dtype=np.uint8).transpose(2, 0, 1).copy()
        return (torch.from_numpy(a).float() / 255.0).cuda()
    for i, v in enumerate(per):
        again = float(metrics.ssim_fn(load(out / "estimates" / f"{i}.png"), load(out / "ground_truth" / f"{i}.png")))
        assert abs(again - v) <= 5.1e-5, (i, again, v)

    plain = run_test_py("--task", "deblurring")
    assert "SSIM: nan" in plain and "SSIM std: nan" in plain and "N: 2" in plain

    sr = run_test_py("--task", "sr", "--sr_factor", "2", "--model_kind", "Upsample", "--ssim")
    assert "N: 2" in sr
    assert math.isfinite(summary(sr, "PSNR")) and math.isfinite(summary(sr, "SSIM"))
