"""GPU: LPIPS on the sei_lpips_* kernels (through metrics.lpips_fn and LPIPS.features) against the float64 restatement of
tests/lpips_ref.py with synthetic weights, its closed forms, determinism and batch independence, and test.py's two flags
end to end."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics
from lpips_ref import features_ref, lpips_ref, pair, synthetic_state_dicts, write_files

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dicts():
    return synthetic_state_dicts()


@pytest.fixture(scope="module")
def files(dicts, tmp_path_factory):
    return write_files(tmp_path_factory.mktemp("lpips"), *dicts, prefix="net.")


@pytest.fixture(scope="module")
def net(files):
    return metrics.LPIPS.from_files(*files, device="cuda")


@pytest.mark.parametrize("s", [0.02, 0.2])
@pytest.mark.parametrize("B,H,W", [(1, 31, 31), (2, 35, 47), (2, 64, 64), (1, 97, 131), (1, 256, 385)])
def test_value_matches_float64_restatement(dicts, net, B, H, W, s):
    """Per image within 1e-5 absolute of float64 (the bar of the SSIM kernel; the driver prints four decimals)."""
    x_hat, x = pair(B, H, W, s, seed=H * 1000 + W)
    ref = lpips_ref(*dicts, x_hat, x)
    got = metrics.lpips_fn(x_hat.cuda(), x.cuda(), net).cpu()
    assert got.shape == (B,) and got.dtype == torch.float32
    err = (got.double() - ref).abs()
    print(f"lpips {B}x{H}x{W} s={s}: values {[round(v, 6) for v in ref.tolist()]}, max |gpu - float64| = "
          f"{float(err.max()):.2e} abs, {float((err / ref).max()):.2e} rel")
    assert float(err.max()) < 1e-5


@pytest.mark.parametrize("B,H,W", [(2, 35, 47), (1, 97, 131)])
def test_feature_maps_match_float64_restatement(dicts, net, B, H, W):
    """The five maps, max-norm error relative to each map's max-abs, at most 4x the error of the same chain through float32
    F.conv2d on the CPU (the matrix instructions accumulate along K in another order than the CPU's blocked sums)."""
    x = pair(B, H, W, 0.1, seed=H * 1000 + W + 1)[1]
    ref = features_ref(dicts[0], x, torch.float64)
    cpu32 = features_ref(dicts[0], x, torch.float32)
    got = net.features(x.cuda())
    worst = []
    for l in range(5):
        assert got[l].shape == ref[l].shape
        scale = float(ref[l].abs().max())
        e_gpu = float((got[l].cpu().double() - ref[l]).abs().max()) / scale
        e_cpu = float((cpu32[l].double() - ref[l]).abs().max()) / scale
        print(f"features {B}x{H}x{W} layer {l}: gpu {e_gpu:.2e}, float32 cpu {e_cpu:.2e} (relative to max-abs {scale:.3f})")
        worst.append((l, e_gpu, e_cpu))
    for l, e_gpu, e_cpu in worst:
        assert e_gpu <= 4 * e_cpu, (l, e_gpu, e_cpu)


def test_zero_image_against_a_random_one(dicts, net):
    """conv1's zero padding pads the SCALED image: with x = 0 every in-image tap is scaled(0) = -2.1 .. -1.8 and every padded
    tap is 0, at every border of the 8 x 11 map."""
    x = pair(1, 35, 47, 0.1, seed=11)[1]
    zero = torch.zeros_like(x)
    ref = float(lpips_ref(*dicts, zero, x)[0])
    got = float(metrics.lpips_fn(zero.cuda(), x.cuda(), net)[0])
    print(f"lpips zero vs random 35x47: {got:.8f} vs float64 {ref:.8f}")
    assert abs(got - ref) < 1e-5


def test_identity_symmetry_and_repeatability(net):
    a, b = (t.cuda() for t in pair(2, 64, 64, 0.2, seed=13))
    assert torch.equal(metrics.lpips_fn(a, a.clone(), net), torch.zeros(2, device="cuda"))
    ab, ba = metrics.lpips_fn(a, b, net), metrics.lpips_fn(b, a, net)
    assert torch.equal(ab, ba) and float(ab.min()) > 0
    assert torch.equal(ab, metrics.lpips_fn(a, b, net))
    one = metrics.lpips_fn(a[1], b[1], net)
    assert one.dim() == 0 and torch.equal(one, ab[1])


def test_batch_equals_its_single_image_calls(net):
    a, b = (t.cuda() for t in pair(4, 64, 64, 0.1, seed=17))
    whole = metrics.lpips_fn(a, b, net)
    singles = torch.stack([metrics.lpips_fn(a[i], b[i], net) for i in range(4)])
    assert torch.equal(whole, singles)


def test_input_at_a_storage_offset_and_dtype_errors(net):
    x_hat, x = pair(2, 35, 47, 0.1, seed=19)
    buf = torch.zeros(1 + x.numel(), device="cuda")
    buf[1:] = x.flatten().cuda()
    xv = buf[1:].view(2, 3, 35, 47)                    # contiguous, 4 bytes off the 16-byte grid
    assert xv.data_ptr() % 16 != 0
    aligned = metrics.lpips_fn(x_hat.cuda(), x.cuda(), net)
    assert torch.equal(metrics.lpips_fn(x_hat.cuda(), xv, net), aligned)
    assert torch.equal(metrics.lpips_fn(xv, x_hat.cuda(), net), aligned)
    with pytest.raises(TypeError):
        metrics.lpips_fn(x_hat.cuda().double(), x.cuda().double(), net)
    with pytest.raises(ValueError):
        metrics.lpips_fn(torch.rand(3, 30, 31).cuda(), torch.rand(3, 30, 31).cuda(), net)


COMMON = ["--device", "cuda", "--dataset", "synthetic", "--kernel", "Gaussian_R2", "--ProposedModel__architecture",
          "Convolutional", "--ConvolutionalModel__hidden_channels", "8", "--ConvolutionalModel__scales", "3", "--indices",
          "0,1", "--task", "deblurring"]


def run_test_py(*flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), *COMMON, *flags], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip().splitlines()


def summary(lines, key):
    return float([ln for ln in lines if ln.startswith(key + ":")][0].split()[-1])


def test_test_py_lpips_flags(files, net, tmp_path):
    from PIL import Image
    out = tmp_path / "eval"
    lines = run_test_py("--lpips_backbone", files[0], "--lpips_linear", files[1], "--print_all_metrics", "--save_images",
                        "--out_dir", str(out))
    per = [float(ln.split("LIPS:")[1]) for ln in lines if ln.startswith("METRICS_")]
    assert len(per) == 2 and all(math.isfinite(v) for v in per)
    assert math.isfinite(summary(lines, "LPIPS")) and math.isfinite(summary(lines, "LPIPS std"))
    assert abs(summary(lines, "LPIPS") - np.mean(per)) < 1e-4

    def load(p):                                   # the 8-bit images the metrics saw, exactly
        a = np.asarray(Image.open(p), dtype=np.uint8).transpose(2, 0, 1).copy()
        return (torch.from_numpy(a).float() / 255.0).cuda()
    for i, v in enumerate(per):
        again = float(metrics.lpips_fn(load(out / "estimates" / f"{i}.png"), load(out / "ground_truth" / f"{i}.png"), net))
        assert abs(again - v) <= 5.1e-5, (i, again, v)          # the four printed decimals

    plain = run_test_py()
    assert "LPIPS: nan" in plain and "LPIPS std: nan" in plain and "N: 2" in plain
