"""LPIPS on the host: the state-dict key handling, metrics.lpips_fn's CPU path against the float64 restatement of
tests/lpips_ref.py, argument errors, test.py's two flags, and the entry points' host-side argument checks (no GPU needed)."""
import importlib.util
import math
import os

import pytest
import torch

import metrics
from lpips_ref import lpips_ref, pair, synthetic_state_dicts, write_files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dicts():
    return synthetic_state_dicts()


@pytest.fixture(scope="module")
def net(dicts, tmp_path_factory):
    pb, pl = write_files(tmp_path_factory.mktemp("lpips"), *dicts)
    return metrics.LPIPS.from_files(pb, pl, device="cpu")


def test_prefixed_keys_load_and_classifier_is_ignored(dicts, tmp_path):
    backbone, linear = dicts
    for prefix in ("net.", "module."):
        pb, pl = write_files(tmp_path, backbone, linear, prefix=prefix)
        got = metrics.LPIPS.from_files(pb, pl, device="cpu")
        for l in range(5):
            assert torch.equal(got.lin[l], linear[f"lin{l}.model.1.weight"])
        assert torch.equal(got.conv_w[1], backbone["features.3.weight"])
        assert torch.equal(got.conv_b[4], backbone["features.10.bias"])
    extra = dict(linear, **{"net.scaling_layer.shift": torch.zeros(1, 3, 1, 1)})
    metrics.LPIPS.from_state_dicts({"module." + k: v for k, v in backbone.items()}, extra)


def test_missing_key_and_wrong_shape_are_named(dicts):
    backbone, linear = dicts
    short = {k: v for k, v in backbone.items() if k != "features.6.bias"}
    with pytest.raises(ValueError, match=r"features\.6\.bias.*\(384,\)"):
        metrics.LPIPS.from_state_dicts(short, linear)
    bad = dict(linear, **{"lin1.model.1.weight": torch.rand(1, 64, 1, 1)})
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight.*\(1, 192, 1, 1\)"):
        metrics.LPIPS.from_state_dicts(backbone, bad)


@pytest.mark.parametrize("B,H,W", [(1, 31, 31), (2, 35, 47)])
def test_host_path_matches_float64_restatement(dicts, net, B, H, W):
    for s in (0.02, 0.2):
        x_hat, x = pair(B, H, W, s, seed=H * 1000 + W)
        ref = lpips_ref(*dicts, x_hat, x)
        got = metrics.lpips_fn(x_hat, x, net)
        assert got.shape == (B,) and got.dtype == torch.float32
        err = float((got.double() - ref).abs().max())
        print(f"lpips host {B}x{H}x{W} s={s}: values {ref.tolist()}, max |f32 - f64| = {err:.2e}")
        assert err < 1e-5
        one = metrics.lpips_fn(x_hat[0], x[0], net)
        assert one.dim() == 0 and abs(float(one) - float(ref[0])) < 1e-5
        assert metrics.lpips_fn(x_hat.double(), x.double(), net).dtype == torch.float64


def test_identical_images_give_exactly_zero(net):
    x = pair(2, 35, 47, 0.1, seed=3)[1]
    assert torch.equal(metrics.lpips_fn(x, x.clone(), net), torch.zeros(2))


def test_small_extents_and_bad_shapes_raise(net):
    for bad in ((3, 30, 31), (3, 31, 30), (2, 3, 30, 40)):
        with pytest.raises(ValueError):
            metrics.lpips_fn(torch.rand(bad), torch.rand(bad), net)
    with pytest.raises(ValueError):
        metrics.lpips_fn(torch.rand(3, 31, 31), torch.rand(3, 31, 32), net)
    with pytest.raises(ValueError):
        metrics.lpips_fn(torch.rand(4, 31, 31), torch.rand(4, 31, 31), net)       # not RGB
    with pytest.raises(ValueError):
        net.features(torch.rand(3, 30, 31))


def test_features_are_the_five_relu_outputs(dicts, net):
    from lpips_ref import features_ref
    x = pair(2, 35, 47, 0.1, seed=5)[1]
    got, ref = net.features(x), features_ref(dicts[0], x)
    assert [tuple(f.shape) for f in got] == [(2, 64, 8, 11), (2, 192, 3, 5), (2, 384, 1, 2), (2, 256, 1, 2), (2, 256, 1, 2)]
    for f, r in zip(got, ref):
        assert float((f.double() - r).abs().max()) < 1e-5 * float(r.abs().max())


def test_compute_metrics_lpips_argument(dicts, net):
    x_hat, x = pair(1, 40, 52, 0.05, seed=7)
    psnr, ssim, lp = metrics.compute_metrics(x[0], x_hat[0])
    assert math.isfinite(psnr) and math.isnan(ssim) and math.isnan(lp)
    assert math.isnan(metrics.compute_metrics(x[0], x_hat[0], ssim=True)[2])
    psnr2, ssim2, lp2 = metrics.compute_metrics(x[0], x_hat[0], lpips=net)
    assert psnr2 == psnr and math.isnan(ssim2)
    assert abs(lp2 - float(lpips_ref(*dicts, x, x_hat)[0])) < 1e-5


def _driver():
    spec = importlib.util.spec_from_file_location("sei_test_driver", os.path.join(ROOT, "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_refuses_one_flag_without_the_other(capsys):
    driver = _driver()
    for given, other in (("--lpips_backbone", "--lpips_linear"), ("--lpips_linear", "--lpips_backbone")):
        with pytest.raises(SystemExit):
            driver.parse_args([given, "weights.pth"])
        assert other in capsys.readouterr().err
    args = driver.parse_args(["--lpips_backbone", "a.pth", "--lpips_linear", "b.pth"])
    assert (args.lpips_backbone, args.lpips_linear) == ("a.pth", "b.pth")
    args = driver.parse_args([])
    assert args.lpips_backbone is None and args.lpips_linear is None


def test_entry_points_refuse_bad_arguments_on_the_host():
    import _native
    L = _native.lib()
    assert L.sei_lpips_conv_relu(None, None, 1, None, None, None, 0, 1, 31, 31, None) == 10001
    assert L.sei_lpips_conv_relu(16, 16, 1, 16, 16, 16, 0, 2, 30, 31, None) == 10001       # below AlexNet's second pool
    assert L.sei_lpips_conv_relu(16, 16, 1, 16, 16, 16, 0, 2, 31, 30, None) == 10001
    assert L.sei_lpips_conv_relu(16, 16, 1, 16, 16, 16, 5, 2, 31, 31, None) == 10001       # layers are 0 .. 4
    assert L.sei_lpips_conv_relu(16, 16, 1, 16, 16, 16, 0, 0, 31, 31, None) == 10001       # no images
    assert L.sei_lpips_conv_relu(16, None, 1, 16, 16, 16, 0, 2, 31, 31, None) == 10001     # split < n without x2
    assert L.sei_lpips_conv_relu(20, None, 2, 16, 16, 16, 1, 2, 31, 31, None) == 10001     # maps are 16-byte aligned
    assert L.sei_lpips_maxpool(None, None, 0, 1, 31, 31, None) == 10001
    assert L.sei_lpips_maxpool(16, 32, 0, 1, 30, 31, None) == 10001
    assert L.sei_lpips_maxpool(16, 32, 2, 1, 31, 31, None) == 10001                        # only layers 0 and 1 are pooled
    assert L.sei_lpips_layer_dist(None, None, None, 0, 1, 31, 31, None, 0, None, None) == 10001
    assert L.sei_lpips_layer_dist(16, 16, 16, 0, 1, 30, 31, 16, 0, 32, None) == 10001
    assert L.sei_lpips_layer_dist(16, 16, 16, 0, 1, 31, 30, 16, 0, 32, None) == 10001
    assert L.sei_lpips_layer_dist(16, 16, 16, 0, 0, 31, 31, 16, 0, 32, None) == 10001
    assert L.sei_lpips_layer_dist(16, 16, 16, 0, 1, 31, 31, 16, 0, None, None) == 10001    # no workspace
    for bad in ((1, 30, 31), (1, 31, 30), (0, 31, 31), (1, 40000, 40)):
        assert L.sei_lpips_work_floats(*bad) == 0
    # 31 x 31: maps 7 x 7 x 64, pooled 3 x 3 x 64, 3 x 3 x 192, pooled 1 x 1 x 192, then 1 x 1 x 384 / 256 / 256
    per_image = 49 * 64 + 9 * 64 + 9 * 192 + 192 + 384 + 256 + 256
    assert L.sei_lpips_work_floats(1, 31, 31) == 2 * per_image + 1024
    assert L.sei_lpips_work_floats(3, 31, 31) == 3 * (2 * per_image + 1024)
