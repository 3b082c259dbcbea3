"""The PlugAndPlay baseline without a GPU: the DPIR schedule's closed forms, conjugate gradients against a dense solve, the
DRUNet key manifest, the onesplit index arithmetic, the model factory's refusals, the host-side argument checks of the
sei_drunet_* entry points, and the refusal of CPU tensors. tests/test_pnp_baseline_gpu.py runs the kernels."""
import math

import pytest
import torch

from drunet_ref import DRUNetRef, dpir_params, synthetic_state_dict


@pytest.mark.parametrize("noise_level", [5, 0])
def test_dpir_schedule_closed_forms(noise_level):
    from models.pnp import PnPModel, get_DPIR_params
    s = noise_level / 255 if noise_level else 1e-5           # the reference replaces 0 by 1e-5
    sigma, step, max_iter = get_DPIR_params(s)
    assert max_iter == 8 and len(sigma) == len(step) == 8
    assert sigma[0] == pytest.approx(49 / 255, rel=1e-6) and sigma[-1] == pytest.approx(s, rel=1e-6)
    assert all(a > b for a, b in zip(sigma, sigma[1:]))
    ratio = sigma[1] / sigma[0]                                # a geometric sequence
    assert all(b / a == pytest.approx(ratio, rel=1e-5) for a, b in zip(sigma, sigma[1:]))
    for sk, tk in zip(sigma, step):
        assert tk * 0.23 * max(0.01, s) ** 2 == pytest.approx(sk ** 2, rel=1e-5)
    ref_sigma, ref_step = dpir_params(s)
    assert sigma == pytest.approx(ref_sigma, rel=1e-6) and step == pytest.approx(ref_step, rel=1e-6)
    model = PnPModel(StubPhysics(), noise_level / 255, denoiser=None)
    assert model.sigma_denoiser == sigma and model.stepsize == step and model.max_iter == 8
    assert model.cg_max_iter == 50 and model.cg_tol == 1e-3 and not model.early_stop


def test_conjugate_gradient_against_a_dense_solve():
    from models.pnp import conjugate_gradient
    g = torch.Generator().manual_seed(0)
    m = torch.randn((12, 12), generator=g, dtype=torch.float64)
    spd = m @ m.T + 0.5 * torch.eye(12, dtype=torch.float64)
    b = torch.randn((12,), generator=g, dtype=torch.float64)
    x = conjugate_gradient(lambda v: spd @ v, b, max_iter=50, tol=1e-12)
    want = torch.linalg.solve(spd, b)
    assert float((x - want).abs().max() / want.abs().max()) < 1e-9
    # the stopping test: sqrt(r . r) < tol after the first update when tol is huge; max_iter caps the loop
    one = conjugate_gradient(lambda v: spd @ v, b, max_iter=50, tol=1e9)
    r0 = b
    alpha = (r0 @ r0) / (r0 @ (spd @ r0))
    assert torch.allclose(one, alpha * r0, rtol=1e-12, atol=0)
    two = conjugate_gradient(lambda v: spd @ v, b, max_iter=2, tol=0.0)
    assert float((two - want).abs().max()) > 1e-6


def test_key_manifest():
    from models.drunet import DRUNet, expected_keys
    keys = expected_keys()
    assert len(keys) == 64 and sum(math.prod(s) for s in keys.values()) == 32_640_960
    assert keys["m_head.weight"] == (64, 4, 3, 3) and keys["m_tail.weight"] == (3, 64, 3, 3)
    assert keys["m_down1.4.weight"] == (128, 64, 2, 2) and keys["m_down3.4.weight"] == (512, 256, 2, 2)
    assert keys["m_up3.0.weight"] == (512, 256, 2, 2) and keys["m_up1.0.weight"] == (128, 64, 2, 2)      # (Cin, Cout, 2, 2)
    assert keys["m_body.3.res.2.weight"] == (512, 512, 3, 3) and keys["m_up2.4.res.0.weight"] == (128, 128, 3, 3)
    assert "m_up2.0.res.0.weight" not in keys and "m_down2.4.res.0.weight" not in keys
    # the independent restatement and the model itself carry exactly these tensors
    assert {k: tuple(v.shape) for k, v in DRUNetRef().state_dict().items()} == keys
    small = DRUNet(nb=1)
    assert {k: tuple(v.shape) for k, v in small.state_dict().items()} == expected_keys(nb=1)
    assert len(expected_keys(nb=1)) == 22 and not any(p.requires_grad for p in small.parameters())
    with pytest.raises(ValueError):
        DRUNet(nc=(64, 128, 256, 500))


def test_onesplit_index_arithmetic():
    from models.drunet import onesplit_plan, piece_extent, runnable
    assert (piece_extent(68), piece_extent(75), piece_extent(256), piece_extent(385)) == (64, 64, 192, 256)
    for h, w in ((68, 75), (256, 385)):
        assert not runnable(h, w)
        ph, pw = piece_extent(h), piece_extent(w)
        plan = onesplit_plan(h, w)
        assert len(plan) == 4
        image = torch.arange(h * w, dtype=torch.float64).view(h, w)
        out = torch.full((h, w), -1.0, dtype=torch.float64)
        for prow, pcol, orow, ocol, irow, icol in plan:
            piece = image[prow, pcol]
            assert piece.shape == (ph, pw) and runnable(ph, pw)
            assert prow.start in (0, h - ph) and pcol.start in (0, w - pw)
            assert (out[orow, ocol] == -1).all()                   # the quadrants do not overlap
            out[orow, ocol] = piece[irow, icol]
        assert torch.equal(out, image)                             # ... cover the image, each pixel from its own place
        assert [(p[2].start, p[3].start) for p in plan] == [(0, 0), (0, w // 2), (h // 2, 0), (h // 2, w // 2)]
    assert runnable(32, 40) and runnable(256, 384) and not runnable(24, 40) and not runnable(40, 57)
    with pytest.raises(ValueError):
        onesplit_plan(40, 75)                                       # 64-row pieces in a 40-row image


def _args(*flags, drunet_weights=None):
    from settings import DefaultArgParser
    args = DefaultArgParser().parse_args(list(flags))
    args.drunet_weights = drunet_weights
    return args


class StubPhysics:
    task = "deblurring"


def test_get_model_refusals(tmp_path):
    from models import get_model
    flags = ("--task", "deblurring", "--kernel", "Gaussian_R2", "--model_kind", "PlugAndPlay")
    with pytest.raises(NotImplementedError, match="drunet_weights"):
        get_model(_args(*flags), physics=StubPhysics(), device="cpu")
    sd = synthetic_state_dict(nb=1)                                 # 22 of the 64 tensors, and one stranger
    sd["m_extra.weight"] = torch.zeros(1)
    path = str(tmp_path / "wrong.pth")
    torch.save(sd, path)
    with pytest.raises(KeyError) as info:
        get_model(_args(*flags, drunet_weights=path), physics=StubPhysics(), device="cpu")
    assert "m_down1.1.res.0.weight" in str(info.value) and "m_extra.weight" in str(info.value)
    assert "Missing" in str(info.value) and "Unexpected" in str(info.value)
    for kind in ("BM3D", "DiffPIR_DRUNet", "DiffPIR_DiffUNet", "DPS"):
        with pytest.raises(NotImplementedError):
            get_model(_args("--task", "deblurring", "--model_kind", kind, drunet_weights=path), physics=None, device="cpu")


def test_pnp_model_has_an_empty_state_dict():
    from models.drunet import DRUNet
    from models.pnp import PnPModel
    net = DRUNet(nb=1)
    model = PnPModel(StubPhysics(), 5 / 255, net, early_stop=True)
    assert len(model.state_dict()) == 0 and list(model.parameters()) == [] and model.denoiser is net and model.early_stop


P, Q = 4096, 4104                # fake device pointers, never dereferenced: 16-byte aligned / 8 off


def test_entry_points_check_their_arguments_on_the_host():
    import _native
    L = _native.lib()
    assert len(_native.SIGNATURES["sei_drunet_conv3x3"]) == 13 and len(_native.SIZE_QUERIES["sei_drunet_work_bytes"]) == 3
    conv = dict(X=P, Wt=P, Cin=64, Cout=128, B=1, H=8, W=8, epilogue=0, T_in=None, T_skip=None, T_out=None, Y16=2 * P, stream=None)
    res = dict(conv, epilogue=1, T_in=P, T_out=P)
    ex = lambda d, pb: dict({k: v for k, v in d.items() if k != "stream"}, pb=pb, stream=None)      # noqa: E731
    refusals = {
        "sei_drunet_conv3x3": [
            (conv, [dict(X=None), dict(Wt=None), dict(Y16=None), dict(Y16=P), dict(X=Q), dict(Wt=Q), dict(Y16=Q), dict(Cin=96),
                    dict(Cout=32), dict(Cin=0), dict(B=0), dict(H=0), dict(W=-1), dict(epilogue=2), dict(epilogue=-1),
                    dict(T_in=P), dict(T_skip=P), dict(T_out=P), dict(H=1 << 20)]),
            (res, [dict(T_in=None), dict(T_out=None), dict(T_in=Q), dict(T_skip=Q), dict(T_out=Q)])],
        "sei_drunet_conv3x3_ex": [
            (ex(conv, 0), [dict(pb=3), dict(pb=8), dict(pb=-1), dict(X=None), dict(Cin=96)]),
            (ex(res, 4), [dict(pb=5), dict(T_in=None), dict(T_out=Q)])],
        "sei_drunet_down": [
            (dict(X=P, Wt=P, Cin=64, Cout=128, B=1, Ho=4, Wo=4, T_out=P, Y16=2 * P, stream=None),
             [dict(X=None), dict(Wt=None), dict(T_out=None), dict(Y16=None), dict(Y16=P), dict(X=Q), dict(T_out=Q), dict(Cin=4),
              dict(Cout=1024), dict(B=0), dict(Ho=0), dict(Wo=0), dict(Ho=16384)])],
        "sei_drunet_up": [
            (dict(X=P, Wt=P, Cin=128, Cout=64, B=1, H=4, W=4, T_out=P, Y16=2 * P, stream=None),
             [dict(X=None), dict(Wt=None), dict(T_out=None), dict(Y16=None), dict(Y16=P), dict(Wt=Q), dict(Y16=Q), dict(Cin=100),
              dict(Cout=0), dict(B=-1), dict(H=0), dict(W=0), dict(W=16384)])],
        "sei_drunet_head": [
            (dict(x=P, sigma=0.05, Wt=P, Cout=64, B=1, H=8, W=8, T_out=P, Y16=2 * P, work=3 * P, stream=None),
             [dict(x=None), dict(Wt=None), dict(T_out=None), dict(Y16=None), dict(work=None), dict(x=P + 2), dict(Wt=Q),
              dict(work=Q), dict(sigma=math.nan), dict(Cout=3), dict(B=0), dict(H=0), dict(W=0)])],
        "sei_drunet_tail": [
            (dict(X=P, Wt=P, Cin=64, B=1, H=8, W=8, out=P, stream=None),
             [dict(X=None), dict(Wt=None), dict(out=None), dict(X=Q), dict(Wt=Q), dict(out=P + 2), dict(Cin=3), dict(B=0),
              dict(H=0), dict(W=0)])],
    }
    for name, groups in refusals.items():
        fn = getattr(L, name)
        for accepted, changes in groups:
            assert len(accepted) == len(_native.SIGNATURES[name])
            for change in changes:
                assert set(change) <= set(accepted)
                assert fn(*dict(accepted, **change).values()) == 10001, f"{name} accepted {change}"
    # the head's workspace: its 32-channel bf16 input grid with W + 3 guard rows on either side
    assert L.sei_drunet_work_bytes(2, 9, 13) == (2 * 11 * 15 + 2 * 16) * 32 * 2
    assert L.sei_drunet_work_bytes(1, 256, 384) == (258 * 386 + 2 * 387) * 64
    for B, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (1, 1 << 20, 8), (1 << 12, 16384, 16384)):
        assert L.sei_drunet_work_bytes(B, H, W) == 0


def test_cpu_tensors_are_refused():
    import _native
    from models.drunet import DRUNet
    from models.pnp import PnPModel
    net = DRUNet(nb=1)
    for mode in ("bf16", "f32"):
        net.compute_dtype = mode
        with pytest.raises(_native.NativeLibraryError):
            net(torch.rand(1, 3, 32, 32), 0.05)
    with pytest.raises(_native.NativeLibraryError):
        PnPModel(StubPhysics(), 5 / 255, net)(torch.rand(1, 3, 32, 32))
    with pytest.raises(TypeError):
        net("not a tensor", 0.05)
