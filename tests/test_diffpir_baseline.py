"""The DiffPIR_DRUNet baseline without a GPU: the tables and the noise schedule against the restatement of
tests/diffpir_ref.py, the model factory's refusals, the refusal of a zero noise level, the empty state dict, and the host-side
argument checks of the sei_cg_* / sei_diffpir_sample entry points. tests/test_diffpir_baseline_gpu.py runs the kernels."""
import math

import numpy as np
import pytest
import torch

from diffpir_ref import nearest_ref, schedule_ref, tables_ref
from drunet_ref import synthetic_state_dict


class Noise:
    def __init__(self, sigma):
        self.sigma = sigma


class StubPhysics:
    task = "deblurring"

    def __init__(self, sigma=5 / 255):
        self.noise_model = Noise(sigma)


_AC = np.cumprod(1.0 - np.linspace(1e-4, 2e-2, 1000))
CANCEL = 1e-6 * _AC / (2 * (1 - _AC)) + 1e-5          # relative allowance on sqrt(1 - ac) for 1e-6 on ac, see below


def test_tables_against_the_restatement():
    from models.diffpir import tables
    tb = tables()
    sa, s1m, red, srec = tables_ref()
    assert all(v.dtype == np.float32 and v.shape == (1000,) for v in tb.values())
    assert tb["betas"][0] == pytest.approx(1e-4, rel=1e-6) and tb["betas"][-1] == pytest.approx(2e-2, rel=1e-6)
    ac = np.cumprod(1.0 - np.linspace(1e-4, 2e-2, 1000))        # float64
    assert np.allclose(tb["ac"], ac, rtol=1e-4)
    # numpy and torch take the float32 cumulative product in their own order: allow 1e-6 of ac (17 ulps over 1000 factors).
    # 1 - ac cancels at small t, so s1m = sqrt(1 - ac) and red = s1m / sa move by that times ac / (2 (1 - ac)).
    for name, ref in (("sa", sa), ("srec", srec)):
        assert np.allclose(tb[name], ref.numpy(), rtol=1e-5, atol=0), name
    for name, ref in (("s1m", s1m), ("red", red)):
        assert np.all(np.abs(tb[name] / ref.numpy() - 1) <= CANCEL), name
    assert np.all(np.diff(tb["red"]) > 0)                       # nearest() is well defined
    assert np.allclose(tb["sa"] ** 2 + tb["s1m"] ** 2, 1.0, atol=1e-6)


@pytest.mark.parametrize("max_iter", [100, 6])
def test_schedule_against_the_restatement(max_iter):
    from models.diffpir import DiffPIR
    sigma = 5 / 255
    model = DiffPIR(StubPhysics(sigma), denoiser=None, max_iter=max_iter)
    rhos, sigmas, seq = schedule_ref(sigma, 7.0, max_iter)
    assert model.seq == seq and len(seq) == max_iter
    assert seq[0] == 0 and seq[-1] == 999 and all(a <= b for a, b in zip(seq, seq[1:]))
    if max_iter == 6:
        assert seq == [0, 447, 632, 774, 894, 999]              # int(sqrt(k / 5) * 1000)
    assert np.all(np.abs(model.rhos / rhos.numpy() - 1) <= 2.5 * CANCEL)            # 1 / red^2
    assert np.all(np.abs(model.sigmas / sigmas.numpy() - 1) <= CANCEL[::-1])
    red64 = np.sqrt(1 - _AC) / np.sqrt(_AC)
    assert np.all(np.abs(model.rhos / (7.0 * sigma ** 2 / red64 ** 2) - 1) <= 2.5 * CANCEL + 1e-4)
    for i in seq:
        cs = float(model.sigmas[i])
        t = model.nearest(cs)
        assert t == nearest_ref(cs) == 999 - i                  # sigmas is red reversed, and red is strictly increasing
        gamma = model.gamma(t)
        assert gamma > 0 and math.isfinite(gamma)
        assert gamma == pytest.approx(1 / (2 * float(rhos[t])), rel=2.5 * CANCEL[t])
    # between two table entries the nearer one wins
    red = model.tables["red"]
    assert model.nearest(0.0) == 0 and model.nearest(1e3) == 999
    assert model.nearest(0.75 * float(red[10]) + 0.25 * float(red[11])) == 10
    assert model.nearest(0.25 * float(red[10]) + 0.75 * float(red[11])) == 11
    assert (model.max_iter, model.zeta, model.lambda_, model.cg_max_iter, model.cg_tol, model.fused_cg) == \
        (max_iter, 0.1, 7.0, 50, 1e-3, True)


def test_defaults_follow_deepinv():
    from models.diffpir import DiffPIR
    model = DiffPIR(StubPhysics(), denoiser=None)
    assert model.max_iter == 100 and len(model.seq) == 100 and model.seq[1] == 100 and model.seq[-2] == 994


def test_zero_noise_level_is_refused():
    from models.diffpir import DiffPIR
    with pytest.raises(ValueError, match="noise"):
        DiffPIR(StubPhysics(0.0), denoiser=None)
    with pytest.raises(ValueError):
        DiffPIR(StubPhysics(), denoiser=None, max_iter=1)


def test_model_has_an_empty_state_dict():
    from models.diffpir import DiffPIR
    from models.drunet import DRUNet
    net = DRUNet(nb=1)
    model = DiffPIR(StubPhysics(), net, max_iter=6)
    assert len(model.state_dict()) == 0 and list(model.parameters()) == [] and model.denoiser is net
    assert model.cg_iterations == []


def _args(*flags, **extra):
    from settings import DefaultArgParser
    args = DefaultArgParser().parse_args(list(flags))
    for k, v in extra.items():
        setattr(args, k, v)
    return args


def test_get_model_builds_and_refuses(tmp_path):
    from models import get_model
    from models.diffpir import DiffPIR
    flags = ("--task", "deblurring", "--kernel", "Gaussian_R2", "--model_kind", "DiffPIR_DRUNet")
    with pytest.raises(NotImplementedError, match="drunet_weights"):
        get_model(_args(*flags), physics=StubPhysics(), device="cpu")
    # both refusals come before the weights file is opened: a file that does not exist is never looked at
    missing = str(tmp_path / "no_such_file.pth")
    with pytest.raises(NotImplementedError, match="physics"):
        get_model(_args(*flags, drunet_weights=missing), physics=None, device="cpu")
    with pytest.raises(NotImplementedError, match="drunet_weights"):
        get_model(_args(*flags, drunet_weights=None), physics=None, device="cpu")
    path = str(tmp_path / "drunet.pth")
    torch.save(synthetic_state_dict(seed=0), path)
    model = get_model(_args(*flags, drunet_weights=path, diffpir_iterations=7), physics=StubPhysics(), device="cpu")
    backbone = model.get_backbone()
    assert isinstance(backbone, DiffPIR) and backbone.max_iter == 7 and len(model.get_weights()) == 0
    assert backbone.sigma == 5 / 255
    assert get_model(_args(*flags, drunet_weights=path), physics=StubPhysics(), device="cpu").get_backbone().max_iter == 100
    with pytest.raises(ValueError, match="noise"):
        get_model(_args(*flags, drunet_weights=path), physics=StubPhysics(0), device="cpu")
    with pytest.raises(ValueError, match="max_iter"):             # (0 is not "not given")
        get_model(_args(*flags, drunet_weights=path, diffpir_iterations=0), physics=StubPhysics(), device="cpu")
    for kind in ("BM3D", "DiffPIR_DiffUNet", "DPS"):
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
    assert driver.parse_args(["--model_kind", "DiffPIR_DRUNet"]).diffpir_iterations == 100
    assert driver.parse_args(["--model_kind", "DiffPIR_DRUNet", "--diffpir_iterations", "4"]).diffpir_iterations == 4


P, Q = 4096, 4104                # fake device pointers, never dereferenced: 16-byte aligned / 8 off


def test_entry_points_check_their_arguments_on_the_host():
    import _native
    L = _native.lib()
    nan, inf = math.nan, math.inf
    refusals = {
        "sei_cg_init": (
            dict(u0=P, Aty=P, inv_gamma=0.5, prologue=0, x=P, r=P, p=P, part=P, state=P, n=105, stream=None),
            [dict(u0=None), dict(Aty=None), dict(x=None), dict(r=None), dict(p=None), dict(part=None), dict(state=None),
             dict(n=0), dict(inv_gamma=nan), dict(inv_gamma=inf), dict(prologue=2), dict(prologue=-1), dict(u0=Q), dict(Aty=Q),
             dict(x=Q), dict(r=Q), dict(p=Q), dict(state=P + 2), dict(part=P + 2)]),
        "sei_cg_apply": (
            dict(p=P, AtAp=P, inv_gamma=0.5, Ap=P, part=P, state=P, n=105, stream=None),
            [dict(p=None), dict(AtAp=None), dict(Ap=None), dict(part=None), dict(state=None), dict(n=0), dict(inv_gamma=nan),
             dict(inv_gamma=-inf), dict(p=Q), dict(AtAp=Q), dict(Ap=Q)]),
        "sei_cg_update": (
            dict(x=P, r=P, p=P, Ap=P, tol=1e-3, part=P, state=P, n=105, stream=None),
            [dict(x=None), dict(r=None), dict(p=None), dict(Ap=None), dict(part=None), dict(state=None), dict(n=0),
             dict(tol=nan), dict(tol=-1.0), dict(tol=inf), dict(x=Q), dict(r=Q), dict(p=Q), dict(Ap=Q)]),
        "sei_cg_direction": (
            dict(p=P, r=P, state=P, n=105, stream=None),
            [dict(p=None), dict(r=None), dict(state=None), dict(n=0), dict(p=Q), dict(r=Q)]),
        "sei_diffpir_sample": (
            dict(u=P, x=P, nz=P, xin=P, sa_t=0.9, s1m_t=0.4, sa_n=0.95, s1m_n=0.3, zeta=0.1, at_n=0.9, n=105, stream=None),
            [dict(u=None), dict(x=None), dict(nz=None), dict(xin=None), dict(n=0), dict(sa_t=nan), dict(s1m_t=0.0),
             dict(s1m_t=nan), dict(sa_n=inf), dict(s1m_n=nan), dict(zeta=-0.1), dict(zeta=1.5), dict(zeta=nan), dict(at_n=0.0),
             dict(at_n=nan), dict(u=Q), dict(x=Q), dict(nz=Q), dict(xin=Q)]),
    }
    for name, (accepted, changes) in refusals.items():
        fn = getattr(L, name)
        assert len(accepted) == len(_native.SIGNATURES[name]), name
        for change in changes:
            assert set(change) <= set(accepted)
            assert fn(*dict(accepted, **change).values()) == 10001, f"{name} accepted {change}"
    # the partials of a reduction: one per workgroup of 256 quads, at least one, at most 1024; a function of n alone
    assert [L.sei_cg_partials(n) for n in (0, 1, 3, 105, 1024, 1025, 4653, 6720, 73731, 294912, 1 << 24)] == \
        [0, 1, 1, 1, 1, 1, 5, 7, 72, 288, 1024]


def test_cpu_tensors_are_refused():
    import _native
    from models.diffpir import DiffPIR
    model = DiffPIR(StubPhysics(), denoiser=None, max_iter=6)
    with pytest.raises(_native.NativeLibraryError):
        model(torch.rand(1, 3, 32, 32))
