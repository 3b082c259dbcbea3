"""The DiffPIR_DiffUNet baseline without a GPU: the key list of models/diffunet.py against the module tree of
tests/diffunet_ref.py, strict loading, the timestep mapping and the embedding against float64, the wrapper's pad and crop
arithmetic, the model factory with and without --diffunet_weights, the errors of the network and the wrapper, the conditions
on the synthetic fixture (activation range; the one-pass variance that the GroupNorm test must be able to catch) and the
host-side refusals of the sei_adm_* entry points. tests/test_diffunet_baseline_gpu.py runs the kernels."""
import math

import numpy as np
import pytest
import torch

import diffunet_ref as R
from diffpir_ref import tables_ref


class Noise:
    def __init__(self, sigma):
        self.sigma = sigma


class StubPhysics:
    def __init__(self, task="deblurring", sigma=5 / 255, rate=None):
        self.task, self.noise_model = task, Noise(sigma)
        if rate is not None:
            self.rate = rate


def _args(*flags, **extra):
    from settings import DefaultArgParser
    args = DefaultArgParser().parse_args(list(flags))
    for k, v in extra.items():
        setattr(args, k, v)
    return args


@pytest.fixture(scope="module")
def sd():
    return R.synthetic_state_dict(seed=0)


def test_expected_keys_match_the_restatement_and_the_issue():
    from models.diffunet import DiffUNet, expected_keys, plan
    want = {k: tuple(v.shape) for k, v in R.DiffUNetRef().state_dict().items()}
    got = expected_keys()
    assert got == want and list(got) == list(want) and len(got) == 362
    assert sum(math.prod(s) for s in got.values()) == 93_563_910
    assert {k: tuple(v.shape) for k, v in DiffUNet().state_dict().items()} == want
    # the (Cin, Cout) pairs of the 3x3 convolutions and the skip widths are the issue's
    pairs = {(s[2], s[3]) for s in plan() if s[0] == "rb"} | {(s[3], s[3]) for s in plan() if s[0] == "rb"}
    assert pairs == {(128, 128), (128, 256), (256, 256), (256, 512), (512, 512), (1024, 512), (768, 512), (768, 256), (512, 256),
                     (384, 256), (384, 128), (256, 128)}
    assert [s[1] for s in plan() if s[0] == "pop"][::-1] == [128, 128, 128, 128, 128, 256, 256, 256, 256, 512, 512, 512]
    assert [s[1] for s in plan() if s[0] == "attn"] == ["input_blocks.9.1", "middle_block.1", "output_blocks.2.1",
                                                        "output_blocks.3.1"]
    assert "output_blocks.3.2.in_layers.2.weight" in got and "output_blocks.1.1.out_layers.3.bias" in got


def test_strict_loading_names_missing_and_extra_keys(sd, tmp_path):
    from models.diffunet import DiffUNet
    net = DiffUNet()
    net.load_state_dict(sd)
    assert torch.equal(net.state_dict()["middle_block.1.qkv.weight"], sd["middle_block.1.qkv.weight"])
    assert all(not p.requires_grad for p in net.parameters()) and net.compute_dtype == "bf16"
    bad = dict(sd)
    del bad["input_blocks.9.1.qkv.bias"]
    bad["stranger.weight"] = torch.zeros(1)
    with pytest.raises(KeyError) as info:
        net.load_state_dict(bad)
    assert "input_blocks.9.1.qkv.bias" in str(info.value) and "stranger.weight" in str(info.value)
    path = str(tmp_path / "bad.pth")
    torch.save(bad, path)
    with pytest.raises(KeyError):
        DiffUNet.from_file(path, "cpu")


def test_synthetic_weights_leave_nothing_trivial(sd):
    for key, v in sd.items():
        assert float(v.abs().max()) > 0, key
        if v.dim() == 1 and not key.endswith(".bias"):
            assert float((v - 1).abs().max()) > 0.05, key              # GroupNorm affines away from the identity
    x = torch.rand((1, 3, 32, 32), generator=torch.Generator().manual_seed(1)) * 2 - 1
    for t in (8, 258):
        lo, hi = R.assert_activation_range(sd, x, t)
        assert 1e-3 <= lo and hi <= 1e3


def test_timestep_mapping():
    from models.diffunet import timestep_of
    s1m = tables_ref()[1].double().numpy()
    below, above = 0.25 * float(s1m[0]), 1000.0                         # s below s1m[0]; s = 1 - 1.25e-7 above s1m[999]
    for sigma in (below, 0.02, 0.1, 0.5, 2.0, above):
        t, s, alpha = timestep_of(sigma)
        assert (t, s, alpha) == pytest.approx(R.timestep_ref(sigma))
        assert alpha == pytest.approx(1 / (1 + 4 * sigma ** 2)) and s == pytest.approx(2 * sigma * math.sqrt(alpha))
        assert s * s + alpha == pytest.approx(1.0)                       # variance preserving
        assert all(abs(s1m[t] - s) <= abs(s1m[k] - s) for k in (max(t - 1, 0), min(t + 1, 999)))
    assert timestep_of(below)[0] == 0 and 2 * below < s1m[0]
    assert timestep_of(above)[0] == 999 and timestep_of(above)[1] > s1m[999]
    assert timestep_of(0.02)[0] == 8 and timestep_of(0.5)[0] == 258


def test_embedding_against_float64(sd):
    from models.diffunet import timestep_embedding
    for t in (0, 8, 258, 999):
        got, ref = timestep_embedding(t), R.timestep_embedding_ref(t)
        assert got.shape == (1, 128) and got.dtype == torch.float32
        assert float((got.double() - ref).abs().max()) <= 2.0 ** -24
    assert float(timestep_embedding(0)[0, :64].min()) == 1.0 and float(timestep_embedding(0)[0, 64:].abs().max()) == 0.0


def test_pad_and_crop_arithmetic():
    from models.diffpir import DiffPIRDiffUNet, pad_amounts
    for (h, w), task, want in (((40, 56), "deblurring", (24, 8)), ((64, 96), "deblurring", (0, 0)),
                               ((24, 40), "sr", (8, 8)), ((33, 47), "sr", (15, 1)), ((33, 47), "deblurring", (31, 17))):
        assert pad_amounts(h, w, task) == want == R.pad_amounts(h, w, task == "deblurring")
    model = DiffPIRDiffUNet(StubPhysics("deblurring"), denoiser=None, max_iter=5)
    assert model.padded_extents(40, 56) == (64, 64) and model.padded_extents(64, 64) == (64, 64)
    assert len(model.state_dict()) == 0 and model.max_iter == 5
    sr = DiffPIRDiffUNet(StubPhysics("sr", rate=2), denoiser=None)
    assert sr.padded_extents(24, 40) == (32, 48) and sr.max_iter == 100
    with pytest.raises(ValueError, match="reflect"):
        model.padded_extents(16, 64)                                     # pad 16 is not smaller than 16 rows
    with pytest.raises(ValueError, match="reflect"):
        sr.padded_extents(24, 8)
    with pytest.raises(ValueError, match="task"):
        DiffPIRDiffUNet(type("P", (), {"noise_model": Noise(0.02)})(), denoiser=None)
    with pytest.raises(ValueError, match="noise"):
        DiffPIRDiffUNet(StubPhysics(sigma=0.0), denoiser=None)


def test_get_model_builds_with_the_flag_and_refuses_without(sd, tmp_path):
    import models
    from models import get_model
    from models.diffpir import DiffPIRDiffUNet
    from models.diffunet import DiffUNet
    assert models._OUT_OF_SCOPE == ("DiffPIR_DiffUNet",)
    flags = ("--task", "sr", "--sr_factor", "2", "--model_kind", "DiffPIR_DiffUNet")
    for physics in (StubPhysics("sr", rate=2), None):
        with pytest.raises(NotImplementedError, match="outside") as info:
            get_model(_args(*flags), physics=physics, device="cpu")
        assert "--diffunet_weights" in str(info.value)
    path = str(tmp_path / "diffunet.pth")
    torch.save(sd, path)
    with pytest.raises(NotImplementedError, match="physics"):
        get_model(_args(*flags, diffunet_weights=path), physics=None, device="cpu")
    model = get_model(_args(*flags, diffunet_weights=path, diffpir_iterations=7), physics=StubPhysics("sr", rate=2), device="cpu")
    inner = model.get_backbone()
    assert isinstance(inner, DiffPIRDiffUNet) and isinstance(inner.denoiser, DiffUNet)
    assert inner.max_iter == 7 and inner.task == "sr" and len(model.get_weights()) == 0
    assert torch.equal(inner.denoiser.state_dict()["out.2.weight"], sd["out.2.weight"])
    default = get_model(_args(*flags, diffunet_weights=path), physics=StubPhysics("sr", rate=2), device="cpu")
    assert default.get_backbone().max_iter == 100
    import test as driver                                                # the driver's parser has the flag
    assert driver.build_parser().parse_args(["--diffunet_weights", "f.pth"]).diffunet_weights == "f.pth"


def test_network_and_wrapper_errors(sd):
    import _native
    from models.diffpir import DiffPIRDiffUNet
    from models.diffunet import DiffUNet
    net = DiffUNet()
    net.load_state_dict(sd)
    with pytest.raises(TypeError):
        net(torch.rand(1, 3, 32, 32), 0.05)                              # a CPU tensor
    with pytest.raises(_native.NativeLibraryError):
        net(torch.rand(1, 3, 32, 32), 0.05)                              # ... which is the library's refusal as well
    with pytest.raises(TypeError):
        net("not a tensor", 0.05)
    with pytest.raises(_native.NativeLibraryError):
        DiffPIRDiffUNet(StubPhysics(), net)(torch.rand(1, 3, 40, 56))


def test_one_pass_variance_fails_the_groupnorm_bar():
    """The GPU test holds GroupNorm to 4x the error of a float32 two-pass CPU chain on an input of mean 100 and standard
    deviation 1. A one-pass E[x^2] - E[x]^2 float32 chain must exceed that bar there, or the case could not fail."""
    g = torch.Generator().manual_seed(5)
    x = (100 + torch.randn((1, 32, 24, 9, 13), generator=g)).float()    # (B, groups, channels of a group, H, W)
    ref = (x.double() - x.double().mean((2, 3, 4), keepdim=True)) / torch.sqrt(x.double().var((2, 3, 4), unbiased=False, keepdim=True) + 1e-5)
    mean = x.mean((2, 3, 4), keepdim=True)
    two = (x - mean) / torch.sqrt(((x - mean) ** 2).mean((2, 3, 4), keepdim=True) + 1e-5)
    one = (x - mean) / torch.sqrt(((x * x).mean((2, 3, 4), keepdim=True) - mean * mean).clamp_min(0) + 1e-5)
    scale = float(ref.abs().max())
    e_two, e_one = (float((v.double() - ref).abs().max()) / scale for v in (two, one))
    print(f"two-pass {e_two:.2e}, one-pass {e_one:.2e}")
    assert e_one > 4 * e_two


P, Q = 4096, 4104       # fake device pointers for calls that must be refused (never dereferenced): aligned, and 8 off


def test_entry_points_refuse_bad_arguments():
    import _native
    L = _native.lib()
    bad = 10001
    assert L.sei_adm_gn_stats(None, 128, None, 0, 1, 4, 4, 1e-5, P, P, None) == bad
    assert L.sei_adm_gn_stats(P, 100, None, 0, 1, 4, 4, 1e-5, P, P, None) == bad              # no whole groups of 4
    assert L.sei_adm_gn_stats(P, 256, None, 128, 1, 4, 4, 1e-5, P, P, None) == bad            # Cb without Xb
    assert L.sei_adm_gn_stats(P, 128, None, 0, 1, 4, 4, 0.0, P, P, None) == bad
    assert L.sei_adm_gn_stats(P, 128, None, 0, 1, 4, 4, 1e-5, P, None, None) == bad         # no room for the slices
    assert L.sei_adm_gn_part_floats(32, 32) == 64 and L.sei_adm_gn_part_floats(32, 40) == 128 and L.sei_adm_gn_part_floats(0, 4) == 0
    assert L.sei_adm_gn_apply(P, 128, None, 0, P, P, P, None, 1, 1, 5, 4, 1, P, None, None) == bad   # odd extent, down
    assert L.sei_adm_gn_apply(P, 128, None, 0, None, P, P, None, 0, 1, 4, 4, 0, P, None, None) == bad  # affine without stats
    assert L.sei_adm_gn_apply(P, 128, None, 0, P, P, P, None, 1, 1, 4, 4, 3, P, None, None) == bad
    assert L.sei_adm_gn_apply(P, 128, None, 0, P, P, P, None, 1, 1, 4, 4, 0, None, None, None) == bad  # no output
    assert L.sei_adm_pack_image(P, Q, 1, 4, 4, None) == bad
    assert L.sei_adm_conv(P, P, P, 384, 256, 9, 1, 4, 4, None, None, None, None) == bad    # no output
    assert L.sei_adm_conv(P, P, P, 100, 256, 9, 1, 4, 4, None, P, None, None) == bad
    assert L.sei_adm_conv(P, P, P, 384, 200, 9, 1, 4, 4, None, P, None, None) == bad
    assert L.sei_adm_conv(P, P, P, 384, 256, 4, 1, 4, 4, None, P, None, None) == bad
    assert L.sei_adm_conv(P, Q, P, 384, 256, 9, 1, 4, 4, None, P, None, None) == bad
    assert L.sei_adm_conv(P, P, None, 384, 256, 9, 1, 4, 4, None, P, None, None) == bad
    assert L.sei_adm_tail(P, P, P, 128, 1, 0, 4, P, None) == bad
    assert L.sei_adm_attention(P, 500, 1, 4, 4, P, None) == bad
    assert L.sei_adm_attention(P, 512, 0, 4, 4, P, None) == bad
    assert L.sei_adm_attention(None, 512, 1, 4, 4, P, None) == bad
