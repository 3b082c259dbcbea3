"""The BM3D baseline without a GPU: the invariants of the float64 restatement tests/bm3d_ref.py, the model factory (builds
BM3D for a physics with a kernel or a filter, refuses the rest), and the host-side argument checks of the new entry points.
tests/test_bm3d_baseline_gpu.py runs the kernels against the restatement."""
import numpy as np
import pytest
import torch

import bm3d_ref as R


def test_transform_matrices_are_orthonormal():
    D = R.dct_matrix()
    assert np.abs(D @ D.T - np.eye(8)).max() < 1e-14
    assert np.allclose(D[0], np.sqrt(1 / 8))                            # the constant basis function comes first
    for n in (1, 2, 4, 8, 16, 32):
        Hm = R.haar_matrix(n)
        assert np.abs(Hm @ Hm.T - np.eye(n)).max() < 1e-14
        assert np.allclose(Hm[0], 1 / np.sqrt(n))                       # the sum of sums ends in slot 0
        x = np.random.default_rng(n).standard_normal((n, 5))
        assert np.allclose(R.haar(x), Hm @ x, atol=1e-14)
        assert np.allclose(R.haar(R.haar(x), inverse=True), x, atol=1e-14)
    assert np.allclose(R.haar(np.array([3.0, 1.0])), [4 / np.sqrt(2), 2 / np.sqrt(2)])


def test_constant_spectrum_gives_constant_variances():
    for H, W in ((8, 8), (21, 35), (48, 40)):
        v = R.coefficient_variances_ref(np.full((H, W), 0.37))
        assert v.shape == (64,) and np.abs(v - 0.37).max() < 1e-13


def test_reference_positions():
    assert R.positions(8) == [0]
    assert R.positions(9) == [0, 1]
    assert R.positions(16) == [0, 3, 6, 8]
    assert R.positions(21) == [0, 3, 6, 9, 12, 13]
    assert R.positions(35) == [0, 3, 6, 9, 12, 15, 18, 21, 24, 27]
    assert R.positions(35, step=1) == list(range(28)) and R.positions(20, step=5) == [0, 5, 10, 12]


def test_groups_are_sorted_cut_and_in_the_window():
    img = R.smooth_image(21, 35, 3)[0] + 0.02 * np.random.default_rng(3).standard_normal((21, 35))
    for tau, n_max in ((R.TAU_HT, 16), (2e-4, 8), (0.0, 4)):
        pos, counts, dists, gaps, before_cut = R.match_ref(img, tau, n_max)
        assert pos.shape == (60, n_max, 2) and counts.shape == (60,) and gaps.shape == (60,)
        assert np.all(counts <= before_cut) and np.all(before_cut < 2 * counts) and np.all(gaps >= 0)
        refs = [(r, c) for r in R.positions(21) for c in R.positions(35)]
        for g, (r, c) in enumerate(refs):
            n = counts[g]
            assert n >= 1 and n & (n - 1) == 0 and n <= n_max
            assert tuple(pos[g, 0]) == (r, c) and dists[g, 0] == 0                    # the block itself comes first
            assert np.all(np.diff(dists[g, :n]) >= 0) and np.all(dists[g, :n] <= tau) and np.all(np.isinf(dists[g, n:]))
            assert np.all(np.abs(pos[g, :, 0] - r) <= 19) and np.all(np.abs(pos[g, :, 1] - c) <= 19)
            assert pos[g, :, 0].min() >= 0 and pos[g, :, 0].max() <= 13 and pos[g, :, 1].min() >= 0 and pos[g, :, 1].max() <= 27
            assert np.all(pos[g, n:] == (r, c))
        if tau == 0.0:
            assert np.all(counts == 1)


def test_zero_threshold_returns_the_input():
    """lambd = 0 keeps every coefficient: the transforms invert and the aggregation is a weighted mean of copies."""
    rng = np.random.default_rng(5)
    img = rng.random((21, 35))
    pos, counts = R.match_ref(img, 0.05, 16)[:2]
    out, margins, _ = R.ht_ref(img, np.full(64, 1e-3), pos, counts, lambd=0.0)
    assert np.abs(out - img).max() < 1e-13 and np.all(np.isinf(margins))


@pytest.fixture(scope="module")
def deblurred():
    from oracle.torch_path import blur_fft, blur_kernel
    x = R.smooth_image(64, 64, 0)[0]
    k = blur_kernel("Gaussian_R2")
    y = blur_fft(torch.from_numpy(x), k).numpy() + 5 / 255 * np.random.default_rng(1).standard_normal(x.shape)
    return x, y, R.deblur_ref(y, k.numpy(), 5 / 255)


def test_restatement_deblurs(deblurred):
    x, y, t = deblurred
    rms = lambda a: float(np.sqrt(((a - x) ** 2).mean()))               # noqa: E731
    print(f"rms to the ground truth: y {rms(y):.4f}, z1 {rms(t['z1']):.4f}, pilot {rms(t['pilot']):.4f}, out {rms(t['out']):.4f}")
    assert rms(t["out"]) < rms(y) and rms(t["out"]) < rms(t["z1"])
    assert np.all(t["v1"] > 0) and np.all(t["v2"] > 0) and np.all(np.isfinite(t["out"]))


def test_restatement_refuses_a_zero_sigma():
    with pytest.raises(ValueError):
        R.deblur_ref(np.zeros((8, 8)), np.ones((3, 3)) / 9, 0.0)


class WithKernel:
    task = "deblurring"
    kernel = torch.ones(1, 1, 5, 5) / 25


class WithFilter:
    task = "deblurring"
    filter = torch.ones(1, 1, 4, 6) / 24


class WithNeither:
    task = "sr"

    def A(self, x):
        return x

    def A_adjoint(self, y):
        return y


def _args(*flags):
    from settings import DefaultArgParser
    return DefaultArgParser().parse_args(list(flags))


def test_get_model_builds_and_refuses():
    import _native
    from models import _OUT_OF_SCOPE, get_model
    from models.bm3d import BM3D
    assert _OUT_OF_SCOPE == ("DiffPIR_DiffUNet",)
    flags = ("--task", "deblurring", "--kernel", "Gaussian_R2", "--model_kind", "BM3D")
    for physics, legacy in ((WithKernel(), False), (WithFilter(), True)):
        model = get_model(_args(*flags), physics=physics, device="cpu")
        backbone = model.get_backbone()
        assert isinstance(backbone, BM3D) and backbone.legacy is legacy
        assert backbone.sigma_psd == pytest.approx(_args(*flags).noise_level / 255)
        assert len(model.get_weights()) == 0 and list(model.parameters()) == []
        model.load_weights({})
        with pytest.raises(_native.NativeLibraryError):                 # no CPU path
            model(torch.rand(1, 3, 16, 16))
    for physics in (None, WithNeither()):
        with pytest.raises(NotImplementedError, match="outside"):
            get_model(_args(*flags), physics=physics, device="cpu")
    with pytest.raises(NotImplementedError, match="outside"):
        get_model(_args("--task", "sr", "--sr_factor", "2", "--model_kind", "BM3D"), physics=WithNeither(), device="cpu")
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="sigma_psd"):
            BM3D(WithKernel(), bad)
    with pytest.raises(ValueError, match="sigma_psd"):
        get_model(_args(*flags, "--noise_level", "0"), physics=WithKernel(), device="cpu")
    with pytest.raises(NotImplementedError, match="outside"):
        get_model(_args("--task", "deblurring", "--model_kind", "DiffPIR_DiffUNet"), physics=WithKernel(), device="cpu")


def test_otf_matches_the_restatement_on_the_cpu():
    """(plain torch plumbing: it runs on any device; the GPU test pins it to the project's own blur operators)"""
    from models.bm3d import coefficient_variances, otf
    g = torch.Generator().manual_seed(2)
    for shape, H, W in (((5, 5), 16, 16), ((4, 6), 21, 35), ((13, 13), 8, 8)):
        k = torch.rand(shape, generator=g)
        got, want = otf(k[None, None], H, W), R.otf_ref(k.numpy(), H, W)
        assert float((got.to(torch.complex128) - want).abs().max()) < 1e-5
    S = torch.rand((2, 21, 35), generator=g)
    got = coefficient_variances(S)
    for p in range(2):
        want = R.coefficient_variances_ref(S[p].numpy().astype(np.float64))
        assert np.abs(got[p].numpy() - want).max() < 1e-5 * want.max()


P, Q = 4096, 4098                # fake device pointers, never dereferenced: aligned / off the 4-byte grid


def test_entry_points_check_their_arguments_on_the_host():
    import _native
    L = _native.lib()
    nan, inf = float("nan"), float("inf")
    shape_bad = [dict(planes=0), dict(H=7), dict(W=7), dict(H=0), dict(W=-8), dict(step=0), dict(step=-3), dict(window=38),
                 dict(window=0), dict(window=-39)]
    n_max_bad = [dict(n_max=n) for n in (0, 3, 5, 12, 24, 64, -16)]
    refusals = {
        "sei_bm3d_match": (
            dict(img=P, planes=3, H=48, W=40, step=3, window=39, tau=0.05, n_max=16, pos=P, counts=P, dist=None, stream=None),
            shape_bad + n_max_bad + [dict(img=None), dict(pos=None), dict(counts=None), dict(img=Q), dict(pos=Q), dict(counts=Q),
                                     dict(dist=Q), dict(tau=-1.0), dict(tau=nan), dict(tau=inf)]),
        "sei_bm3d_ht": (
            dict(noisy=P, var=P, pos=P, counts=P, planes=3, H=48, W=40, step=3, n_max=16, window=39, lambd=2.7, agg=0,
                 work=2 * P, coef=None, stream=None),
            shape_bad + n_max_bad + [dict(noisy=None), dict(var=None), dict(pos=None), dict(counts=None), dict(work=None),
                                     dict(noisy=Q), dict(var=Q), dict(pos=Q), dict(counts=Q), dict(work=Q), dict(coef=Q),
                                     dict(work=P), dict(lambd=-1.0), dict(lambd=nan), dict(lambd=inf), dict(agg=2), dict(agg=-1)]),
        "sei_bm3d_wiener": (
            dict(noisy=P, pilot=P, var=P, pos=P, counts=P, planes=3, H=48, W=40, step=3, n_max=32, window=39, agg=0,
                 work=2 * P, stream=None),
            shape_bad + n_max_bad + [dict(noisy=None), dict(pilot=None), dict(var=None), dict(pos=None), dict(counts=None),
                                     dict(work=None), dict(noisy=Q), dict(pilot=Q), dict(work=Q), dict(work=P), dict(agg=2)]),
        "sei_bm3d_finish": (
            dict(work=P, out=16 * P, planes=3, H=48, W=40, stream=None),
            [dict(work=None), dict(out=None), dict(work=Q), dict(out=Q), dict(out=P), dict(out=P + 3 * 48 * 40 * 4),
             dict(planes=0), dict(H=7), dict(W=0)]),
    }
    for name, (accepted, changes) in refusals.items():
        fn = getattr(L, name)
        assert len(accepted) == len(_native.SIGNATURES[name]), name
        for change in changes:
            assert set(change) <= set(accepted), change
            assert fn(*dict(accepted, **change).values()) == 10001, f"{name} accepted {change}"
    # what does not fit 64 KiB of LDS: the search region of a wide window, the footprint of a tile at a wide step or window
    assert L.sei_bm3d_match(P, 1, 48, 40, 3, 91, 0.05, 16, P, P, None, None) == 10002
    assert L.sei_bm3d_ht(P, P, P, P, 1, 48, 40, 3, 16, 91, 2.7, 0, 2 * P, None, None) == 10002
    assert L.sei_bm3d_ht(P, P, P, P, 1, 480, 400, 20, 16, 39, 2.7, 0, 2 * P, None, None) == 10002
    assert L.sei_bm3d_wiener(P, P, P, P, P, 1, 48, 40, 3, 32, 91, 0, 2 * P, None) == 10002
    # the number of reference blocks: positions 0, step ... and the last one
    assert [L.sei_bm3d_ref_blocks(H, W, s) for H, W, s in ((8, 8, 3), (16, 16, 3), (21, 35, 3), (48, 40, 3), (256, 384, 3),
                                                           (20, 9, 5))] == [1, 16, 60, 180, 84 * 127, 4 * 2]
    assert [L.sei_bm3d_ref_blocks(H, W, s) for H, W, s in ((7, 8, 3), (8, 7, 3), (8, 8, 0), (0, 0, 1))] == [0, 0, 0, 0]
    for H, W in ((8, 8), (16, 16), (21, 35), (48, 40)):
        assert L.sei_bm3d_ref_blocks(H, W, 3) == len(R.positions(H)) * len(R.positions(W))
