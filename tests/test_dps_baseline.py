"""The DPS baseline without a GPU: the tables, the schedule and the step's coefficients against the restatement of
tests/dps_ref.py, the model factory (builds DPS, refuses in the documented order), test.py's flag, the host-side argument
checks of the new entry points, the packing of the transposed weights against autograd, and the restatement's hand-written
transposed network against autograd through its own forward. tests/test_dps_baseline_gpu.py runs the kernels."""
import math

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from dps_ref import (coefficients_ref, mask_flips, masked_network_ref, preactivation_signs_ref, schedule_ref, tables_ref,
                     vjp_ref)
from drunet_ref import assert_activation_range, network_ref, synthetic_state_dict


class StubPhysics:
    task = "deblurring"

    def A(self, x):
        return x

    def A_adjoint(self, y):
        return y


class NoOperators:
    task = "deblurring"


def test_tables_against_the_restatement():
    from models.dps import tables
    betas, ac = tables()
    betas_ref, ac_ref = tables_ref()
    assert betas.dtype == ac.dtype == np.float32 and betas.shape == (1000,) and ac.shape == (1001,)
    assert np.array_equal(betas, betas_ref.numpy())
    assert ac[0] == 1.0 and float(ac_ref[0]) == 1.0                      # alpha(-1) = 1 exactly
    # numpy and torch take the float32 cumulative product in their own order: 1e-6 of ac (17 ulps over 1000 factors)
    assert np.allclose(ac, ac_ref.numpy(), rtol=1e-6, atol=0)
    assert np.allclose(ac[1:], np.cumprod(1.0 - np.linspace(1e-4, 2e-2, 1000)), rtol=1e-4)
    assert np.all(np.diff(ac) < 0)


@pytest.mark.parametrize("max_iter", [1000, 100, 7])
def test_schedule_and_coefficients_against_the_restatement(max_iter):
    from models.dps import DPS
    model = DPS(StubPhysics(), denoiser=None, max_iter=max_iter)
    pairs = schedule_ref(max_iter)
    assert model.pairs == pairs and pairs[-1] == (0, -1) and pairs[0][0] == max(i for i, _ in pairs)
    assert all(i > j for i, j in pairs) and all(a[1] == b[0] for a, b in zip(pairs, pairs[1:]))
    if max_iter == 7:
        assert [i for i, _ in pairs] == [994, 852, 710, 568, 426, 284, 142, 0]      # skip = 142: eight steps
    else:
        assert len(pairs) == max_iter
    for i, j in pairs:
        c = model.coefficients(i, j)
        at, an = model.alpha(i), model.alpha(j)
        sigma, st, c2 = coefficients_ref(at, an)
        assert (c["sigma"], c["st"], c["c2"]) == pytest.approx((sigma, st, c2), rel=1e-12, abs=0)
        assert c["ginv"] == pytest.approx(1 / (2 * math.sqrt(at)), rel=1e-12)
        assert c["c0"] == pytest.approx(math.sqrt(an) - c2 * math.sqrt(at) / math.sqrt(1 - at), rel=1e-12)
        assert c["c1"] == pytest.approx(c2 / math.sqrt(1 - at), rel=1e-12) and c["den"] == pytest.approx(2 * math.sqrt(an))
        assert all(math.isfinite(v) for v in c.values()) and 0 < at < an <= 1
    last = model.coefficients(*pairs[-1])
    assert last["st"] == 0.0 and last["c2"] == 0.0 and last["c1"] == 0.0 and last["c0"] == 1.0 and last["den"] == 2.0
    assert (model.max_iter, model.eta, model.fused) == (max_iter, 1.0, True)


def test_bad_iteration_counts_are_refused():
    from models.dps import DPS
    for bad in (0, -3, 1001):
        with pytest.raises(ValueError, match="max_iter"):
            DPS(StubPhysics(), denoiser=None, max_iter=bad)
    assert DPS(StubPhysics(), denoiser=None).max_iter == 1000
    assert DPS(StubPhysics(), denoiser=None, max_iter=1).pairs == [(0, -1)]


def test_model_has_an_empty_state_dict_and_refuses_cpu_tensors():
    import _native
    from models.dps import DPS
    from models.drunet import DRUNet
    net = DRUNet(nb=1)
    model = DPS(StubPhysics(), net, max_iter=5)
    assert len(model.state_dict()) == 0 and list(model.parameters()) == [] and model.denoiser is net
    with pytest.raises(_native.NativeLibraryError):
        model(torch.rand(1, 3, 32, 32))


def _args(*flags, **extra):
    from settings import DefaultArgParser
    args = DefaultArgParser().parse_args(list(flags))
    for k, v in extra.items():
        setattr(args, k, v)
    return args


def test_get_model_builds_and_refuses(tmp_path):
    from models import get_model
    from models.dps import DPS
    flags = ("--task", "deblurring", "--kernel", "Gaussian_R2", "--model_kind", "DPS")
    with pytest.raises(NotImplementedError, match="drunet_weights"):
        get_model(_args(*flags), physics=StubPhysics(), device="cpu")
    with pytest.raises(NotImplementedError, match="drunet_weights"):       # the flag comes first
        get_model(_args(*flags, drunet_weights=None), physics=None, device="cpu")
    # ... then the physics, both before the weights file is opened: a file that does not exist is never looked at
    missing = str(tmp_path / "no_such_file.pth")
    for physics in (None, NoOperators()):
        with pytest.raises(NotImplementedError, match="A_adjoint.*outside"):
            get_model(_args(*flags, drunet_weights=missing), physics=physics, device="cpu")
    path = str(tmp_path / "drunet.pth")
    torch.save(synthetic_state_dict(seed=0), path)
    model = get_model(_args(*flags, drunet_weights=path, dps_iterations=7), physics=StubPhysics(), device="cpu")
    backbone = model.get_backbone()
    assert isinstance(backbone, DPS) and backbone.max_iter == 7 and len(backbone.pairs) == 8
    assert len(model.get_weights()) == 0
    model.load_weights({})
    assert get_model(_args(*flags, drunet_weights=path), physics=StubPhysics(), device="cpu").get_backbone().max_iter == 1000
    with pytest.raises(ValueError, match="max_iter"):                       # (0 is not "not given")
        get_model(_args(*flags, drunet_weights=path, dps_iterations=0), physics=StubPhysics(), device="cpu")
    for kind in ("BM3D", "DiffPIR_DiffUNet"):
        with pytest.raises(NotImplementedError, match="outside"):
            get_model(_args("--task", "deblurring", "--model_kind", kind, drunet_weights=path), physics=StubPhysics(),
                      device="cpu")


def test_test_py_has_the_iterations_flag():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("sei_test_driver", os.path.join(root, "test.py"))
    driver = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(driver)
    assert driver.parse_args(["--model_kind", "DPS"]).dps_iterations == 1000
    assert driver.parse_args(["--model_kind", "DPS", "--dps_iterations", "4"]).dps_iterations == 4


P, Q = 4096, 4104                # fake device pointers, never dereferenced: 16-byte aligned / 8 off


def test_entry_points_check_their_arguments_on_the_host():
    import _native
    L = _native.lib()
    nan, inf = math.nan, math.inf
    conv = dict(X=P, Wt=2 * P, Cin=64, Cout=64, B=1, H=4, W=5, Mask=3 * P, Y16=4 * P)
    conv_bad = [dict(X=None), dict(Wt=None), dict(Mask=None), dict(Y16=None), dict(Y16=P), dict(Y16=3 * P), dict(X=Q), dict(Wt=Q),
                dict(Mask=Q), dict(Y16=Q), dict(Cin=32), dict(Cin=96), dict(Cout=48), dict(Cout=1024), dict(B=0), dict(H=0),
                dict(W=0), dict(H=16385), dict(B=1 << 20, H=1024, W=1024)]
    refusals = {
        "sei_drunet_conv3x3_masked": (dict(conv, stream=None), conv_bad),
        "sei_drunet_conv3x3_masked_ex": (dict(conv, pb=0, stream=None), conv_bad + [dict(pb=3), dict(pb=-1), dict(pb=8)]),
        "sei_dps_u": (
            dict(out=P, u=2 * P, B=3, m=105, stream=None),
            [dict(out=None), dict(u=None), dict(u=P), dict(B=0), dict(B=65536), dict(m=0), dict(out=Q), dict(u=Q)]),
        "sei_dps_residual": (
            dict(Au=P, y=P, r=P, part=P, f=P, s=2 * P, B=3, m=105, stream=None),
            [dict(Au=None), dict(y=None), dict(r=None), dict(part=None), dict(f=None), dict(s=None), dict(s=P), dict(B=0),
             dict(m=0), dict(Au=Q), dict(y=Q), dict(r=Q), dict(part=P + 2), dict(f=P + 2), dict(s=P + 2)]),
        "sei_dps_seed": (
            dict(Atr=P, out=P, seed=P, B=3, m=105, stream=None),
            [dict(Atr=None), dict(out=None), dict(seed=None), dict(B=0), dict(m=0), dict(Atr=Q), dict(out=Q), dict(seed=Q)]),
        "sei_dps_step": (
            dict(out=P, gx=P, nz=P, s=P, x=2 * P, xin=3 * P, c0=0.5, c1=0.5, st=0.1, ginv=0.6, den=1.9, B=3, m=105, stream=None),
            [dict(out=None), dict(gx=None), dict(nz=None), dict(s=None), dict(x=None), dict(xin=None), dict(x=P), dict(xin=2 * P),
             dict(B=0), dict(m=0), dict(c0=nan), dict(c1=inf), dict(st=nan), dict(ginv=-inf), dict(den=0.0), dict(den=-2.0),
             dict(den=nan), dict(out=Q), dict(gx=Q), dict(nz=Q), dict(x=Q), dict(xin=Q), dict(s=P + 2)]),
    }
    for name, (accepted, changes) in refusals.items():
        fn = getattr(L, name)
        assert len(accepted) == len(_native.SIGNATURES[name]), name
        for change in changes:
            assert set(change) <= set(accepted)
            assert fn(*dict(accepted, **change).values()) == 10001, f"{name} accepted {change}"
    # the partials of the residual's reduction: per image one per workgroup of 256 quads, at least one, at most 1024
    assert [L.sei_dps_partials(B, m) for B, m in ((0, 5), (1, 0), (1, 1), (3, 105), (2, 4653), (1, 1 << 24))] == \
        [0, 0, 1, 3, 10, 1024]


def _input_gradient(fn, x, g):
    x = x.clone().requires_grad_(True)
    return torch.autograd.grad((fn(x) * g).sum(), x)[0]


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_transposed_weights_are_packed_as_autograd_differentiates(mode):
    """For each layer kind: the packed transposed weight, read back as its kernel reads it and applied by a float64
    F.conv2d / F.conv_transpose2d, gives autograd's input gradient of the layer."""
    from models.drunet import DRUNet
    gen = torch.Generator().manual_seed(5)
    rnd = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64)      # noqa: E731
    pack = lambda key, w: DRUNet.pack_transposed(key, w, mode)                       # noqa: E731
    lo, hi = 5, 6
    # a ResBlock's 3x3 convolution
    w, x = rnd(hi, lo, 3, 3), rnd(2, lo, 7, 9)
    g = rnd(2, hi, 7, 9)
    p = pack("m_body.0.res.0.weight", w)
    wt = p.view(3, 3, lo, hi).permute(2, 3, 0, 1) if mode == "f32" else p.view(lo, 3, 3, hi).permute(0, 3, 1, 2)
    assert torch.allclose(F.conv2d(g, wt, padding=1), _input_gradient(lambda v: F.conv2d(v, w, padding=1), x, g), atol=1e-12)
    # the 2x2 stride-2 convolution of a down stage: its transpose is an up layer, (4 Cout, Cin) with row (ky 2 + kx) Cout + co
    w, x = rnd(hi, lo, 2, 2), rnd(2, lo, 6, 8)
    g = rnd(2, hi, 3, 4)
    p = pack("m_down1.4.weight", w)
    assert p.shape == (4 * lo, hi)
    wt = p.view(2, 2, lo, hi).permute(3, 2, 0, 1)                         # ConvTranspose2d's (Cin, Cout, 2, 2)
    assert torch.allclose(F.conv_transpose2d(g, wt, stride=2), _input_gradient(lambda v: F.conv2d(v, w, stride=2), x, g),
                          atol=1e-12)
    # the transposed convolution of an up stage: its transpose is a down layer, tap-major (Cout, 4 Cin)
    w, x = rnd(hi, lo, 2, 2), rnd(2, hi, 3, 4)                            # ConvTranspose2d(hi -> lo)
    g = rnd(2, lo, 6, 8)
    p = pack("m_up1.0.weight", w)
    assert p.shape == (hi, 4 * lo)
    wt = p.view(hi, 2, 2, lo).permute(0, 3, 1, 2)
    assert torch.allclose(F.conv2d(g, wt, stride=2), _input_gradient(lambda v: F.conv_transpose2d(v, w, stride=2), x, g),
                          atol=1e-12)
    # the tail (nc0 -> 3): its transpose runs on the head's kernel (bf16: 32 input channels, 3 live) / the transposed switch
    w, x = rnd(3, hi, 3, 3), rnd(2, hi, 7, 9)
    g = rnd(2, 3, 7, 9)
    want = _input_gradient(lambda v: F.conv2d(v, w, padding=1), x, g)
    p = pack("m_tail.weight", w)
    if mode == "bf16":
        wt = p.view(hi, 3, 3, 32).permute(0, 3, 1, 2)
        assert float(wt[:, 3:].abs().max()) == 0.0
        assert torch.allclose(F.conv2d(g, wt[:, :3], padding=1), want, atol=1e-12)
    else:
        assert torch.allclose(F.conv_transpose2d(g, p, padding=1), want, atol=1e-12)
    # the head (4 -> nc0): its transpose runs on the tail's kernel (bf16: 16 rows, 3 live); the sigma channel gets no gradient
    w, x = rnd(hi, 4, 3, 3), rnd(2, 4, 7, 9)
    g = rnd(2, hi, 7, 9)
    want = _input_gradient(lambda v: F.conv2d(v, w, padding=1), x, g)[:, :3]
    p = pack("m_head.weight", w)
    if mode == "bf16":
        wt = p.view(16, 3, 3, hi).permute(0, 3, 1, 2)
        assert float(wt[3:].abs().max()) == 0.0
        assert torch.allclose(F.conv2d(g, wt[:3], padding=1), want, atol=1e-12)
    else:
        assert torch.allclose(F.conv_transpose2d(g, p, padding=1), want, atol=1e-12)


@pytest.fixture(scope="module")
def fixture():
    """The fixture of the GPU test of the VJP: full widths, nb = 2, x of (2, 3, 32, 40), sigma 0.05."""
    sd = synthetic_state_dict(nb=2, seed=2)
    x = torch.rand((2, 3, 32, 40), generator=torch.Generator().manual_seed(40))
    signs = preactivation_signs_ref(sd, x.double(), 0.05, torch.float64)
    return sd, x, signs


def test_restatement_of_the_transposed_network(fixture):
    """In float64, with the ReLUs fixed to the forward's own signs: the masked network is the network, and the hand-written
    transposed network is autograd's gradient of it."""
    sd, x, signs = fixture
    assert len(signs) == 14 and signs[0].shape == (2, 64, 32, 40) and signs[6].shape == (2, 512, 4, 5)
    xd = x.double().requires_grad_(True)
    out = masked_network_ref(sd, xd, 0.05, signs, torch.float64)
    assert torch.equal(out.detach(), network_ref(sd, x.double(), 0.05, torch.float64))
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(41), dtype=torch.float64)
    want = torch.autograd.grad((out * g).sum(), xd)[0]
    got = vjp_ref(sd, signs, g, torch.float64)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_mask_plausibility_of_the_cpu_chains(fixture):
    """The cap of the GPU test on the device's mask flips against float64 is 4x the CPU chain's count plus 8. A flip needs a
    pre-activation within the chain's error of zero: with errors of 1e-6 (float32) and 1e-2 (bf16 roundings) relative to
    pre-activations of order one, at most a 1e-4 / a 5e-2 share of the units, or the fixture is degenerate."""
    sd, x, signs = fixture
    assert_activation_range(sd, x, 0.05)
    units = sum(s.numel() for s in signs)
    n32 = mask_flips(preactivation_signs_ref(sd, x, 0.05, torch.float32), signs)
    n16 = mask_flips(preactivation_signs_ref(sd, x, 0.05, torch.float32, round_bf16=True), signs)
    print(f"mask flips against float64 over {units} units: float32 chain {n32}, bf16-rounded chain {n16}")
    assert n32 <= 1e-4 * units and n32 <= n16 <= 5e-2 * units
