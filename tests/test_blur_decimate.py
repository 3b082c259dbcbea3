"""The blur-then-decimate operator (physics.BlurDownsampling) on the host: the axis matrices of physics/_bands against a
float64 pad + strided conv and its autograd (tests/blur_decimate_ref.py), their band step, the argument checks of
sei_blur_decimate (made before any HIP call, so they run without a GPU), the get_physics wiring and the flag refusals."""
import argparse

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from blur_decimate_ref import axis_matrix64, conv64, pad_axis_index, rand_kernel

PADDINGS = ("circular", "replicate", "reflect")


def test_the_float64_helper_pads_as_torch_does():
    """The helper gathers the padded image by index (so that it can wrap more than once); where F.pad applies they agree."""
    x = torch.rand(1, 1, 9, 11, dtype=torch.float64)
    for padding in PADDINGS:
        iv, ih = torch.from_numpy(pad_axis_index(9, 3, padding)), torch.from_numpy(pad_axis_index(11, 2, padding))
        assert torch.equal(x[:, :, iv][:, :, :, ih], F.pad(x, (2, 2, 3, 3), mode=padding))
    assert list(pad_axis_index(3, 4, "circular")) == [2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0]


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("K", [5, 4, 1])                       # odd, even and single-tap axes
@pytest.mark.parametrize("n,rate", [(12, 2), (13, 2), (13, 3), (14, 4)])          # n % s == 0 and != 0
def test_axis_matrix_vs_float64_strided_conv(n, rate, K, padding):
    from physics import _bands
    taps = np.random.default_rng(10 * K + rate).random(K)
    for phase in sorted({0, rate - 1}):
        got = _bands.blur_decimate_axis_matrix(n, taps, padding, rate, phase)
        want = axis_matrix64(n, taps, padding, rate, phase)
        n_out = (n - phase + rate - 1) // rate
        assert got.dtype == np.float64 and got.shape == want.shape == (n_out, n)
        assert n_out == len(range(n)[phase::rate])
        assert np.abs(got - want).max() < 1e-15, (n, rate, K, padding, phase)
        assert np.array_equal(got, _bands.blur_axis_matrix(n, taps, padding)[phase::rate])


@pytest.mark.parametrize("padding", PADDINGS)
def test_axis_matrices_give_the_operator_and_its_autograd(padding):
    """M_v x M_h^T is the strided conv in two dimensions, M_v^T g M_h its autograd transpose (a 5 x 4 kernel is not rank
    1, so the 2-D check uses an outer product of two tap vectors)."""
    from physics import _bands
    gen = torch.Generator().manual_seed(4)
    tv, th = torch.rand(5, generator=gen, dtype=torch.float64), torch.rand(4, generator=gen, dtype=torch.float64)
    x = torch.rand((2, 1, 13, 10), generator=gen, dtype=torch.float64).requires_grad_(True)
    for rate, phase in ((2, 0), (3, 2)):
        y = conv64(x, torch.outer(tv, th), padding, rate, phase)
        g = torch.rand(y.shape, generator=gen, dtype=torch.float64)
        (gx,) = torch.autograd.grad(y, x, g)
        mv = torch.from_numpy(_bands.blur_decimate_axis_matrix(13, tv.numpy(), padding, rate, phase))
        mh = torch.from_numpy(_bands.blur_decimate_axis_matrix(10, th.numpy(), padding, rate, phase))
        assert (mv @ x.detach() @ mh.T - y.detach()).abs().max() < 1e-14
        assert (mv.T @ g @ mh - gx).abs().max() < 1e-14


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("rate", [1, 2, 3, 4])
def test_band_step_is_the_rate(rate, padding):
    from physics import _bands
    taps = np.random.default_rng(rate).random(7) + 0.1
    for phase in sorted({0, rate - 1}):
        m = _bands.blur_decimate_axis_matrix(41, taps, padding, rate, phase)
        w, lo, nb, step = _bands.to_band(m)
        if padding == "circular":          # rows that wrap span the whole axis: their band is the row, steps stay <= rate
            assert step <= rate
        else:
            assert step == rate and nb <= 7 + rate, (step, nb)
        # the transposed bands (the exact adjoint) step by at most one measurement pixel per image pixel
        wt, lot, nbt, stept = _bands.to_band(np.ascontiguousarray(m.T))
        assert stept <= 1 or padding == "circular"
        back = np.zeros_like(m)
        for o in range(m.shape[0]):
            back[o, lo[o]:lo[o] + nb] = w[o, :min(nb, m.shape[1] - lo[o])]
        assert np.abs(back - m).max() < 1e-7 * np.abs(m).max()


def test_axis_matrix_refusals():
    from physics import _bands
    with pytest.raises(ValueError, match="valid"):
        _bands.blur_decimate_axis_matrix(12, [0.5, 0.5], "valid", 2)
    with pytest.raises(ValueError, match="phase"):
        _bands.blur_decimate_axis_matrix(12, [0.5, 0.5], "reflect", 2, 2)
    with pytest.raises(ValueError, match="rate"):
        _bands.blur_decimate_axis_matrix(12, [0.5, 0.5], "reflect", 0)
    with pytest.raises(ValueError, match="extent of 3 "):
        _bands.blur_decimate_axis_matrix(3, np.ones(7) / 7, "reflect", 2)


# Fake device pointers for calls that must be refused: never dereferenced, because a refused call launches nothing.
X, Y, K_, WORK = 1 << 20, 2 << 20, 3 << 20, 4 << 20
BAD_ARG, TOO_LARGE = 10001, 10002


def test_entry_point_refuses_bad_arguments_on_the_host():
    import _native
    L = _native.lib()

    def call(x=X, y=Y, k=K_, kv=5, kh=5, planes=2, H=17, W=21, mode=1, rate=2, phase_v=0, phase_h=0, transpose=0, work=WORK):
        return L.sei_blur_decimate(x, y, k, kv, kh, planes, H, W, mode, rate, phase_v, phase_h, transpose, work, None)

    def query(planes=2, H=17, W=21, kv=5, kh=5, mode=1, rate=2, transpose=1):
        return L.sei_blur_decimate_work_floats(planes, H, W, kv, kh, mode, rate, transpose)

    for transpose in (0, 1):
        for null in ("x", "y", "k"):
            assert call(transpose=transpose, **{null: None}) == BAD_ARG
        for mode in (3, 4, -1):                                     # 3 is valid: not part of this operator
            assert call(mode=mode, transpose=transpose) == BAD_ARG and query(mode=mode, transpose=transpose) == 0
        for rate in (0, 9, -2):
            assert call(rate=rate, transpose=transpose) == BAD_ARG and query(rate=rate, transpose=transpose) == 0
        for phases in (dict(phase_v=2), dict(phase_h=2), dict(phase_v=-1), dict(rate=4, phase_h=4)):
            assert call(transpose=transpose, **phases) == BAD_ARG
        for taps in (dict(kv=64), dict(kh=64), dict(kv=64, kh=64)):
            assert call(transpose=transpose, **taps) == TOO_LARGE and query(transpose=transpose, **taps) == 0
        for size in (dict(planes=0), dict(H=0), dict(W=-1), dict(kv=0), dict(kh=0)):
            assert call(transpose=transpose, **size) == BAD_ARG and query(transpose=transpose, **size) == 0
        # reflect needs p <= n - 1
        assert call(mode=2, kv=7, H=3, transpose=transpose) == BAD_ARG and query(mode=2, kv=7, H=3, transpose=transpose) == 0
    assert call(transpose=1, work=None) == BAD_ARG                  # the canvas of replicate / reflect is required ...
    # work: the canvas of the replicate / reflect transposes, nothing otherwise
    assert query() == 2 * (17 + 4) * (21 + 4) and query(mode=2) == 2 * (17 + 4) * (21 + 4)
    assert query(rate=4) == query(rate=1) == query()                 # the canvas is image-sized whatever the rate
    assert query(kv=4, kh=1) == 2 * (17 + 4) * (21 + 2)             # p = (2, 1)
    assert query(mode=2, kv=7, H=4) == 2 * (4 + 6) * (21 + 4)
    assert query(transpose=0) == 0 and query(mode=2, transpose=0) == 0
    assert query(mode=0) == 0 and query(mode=0, transpose=0) == 0    # circular folds its wraps in the kernel
    # overlapping operands: x is the image (2 x 17 x 21) forward, the measurement (2 x 9 x 11) transposed
    n_img, n_meas = 2 * 17 * 21 * 4, 2 * 9 * 11 * 4
    assert call(y=X) == BAD_ARG and call(y=X + n_img - 4) == BAD_ARG and call(y=X - n_meas + 4) == BAD_ARG
    assert call(transpose=1, y=X + n_meas - 4) == BAD_ARG and call(transpose=1, y=X - n_img + 4) == BAD_ARG
    assert call(k=Y + 8) == BAD_ARG and call(mode=0, k=Y + 8) == BAD_ARG
    assert call(transpose=1, work=X + 64) == BAD_ARG and call(transpose=1, work=Y - 16) == BAD_ARG
    assert call(transpose=1, work=K_ - 4) == BAD_ARG


def _args(**over):
    base = dict(task="sr", kernel=None, sr_factor=2, noise_level=5, physics_v2=True, physics_true_adjoint=False)
    base.update(over)
    return argparse.Namespace(**base)


def test_sr_without_the_flag_still_builds_downsampling():
    import physics
    for extra in ({}, dict(sr_kernel=None, sr_phase=0), dict(sr_kernel=None, blur_padding="reflect")):
        p = physics.get_physics(_args(**extra), "cpu")
        assert type(p) is physics.Downsampling and p.rate == 2 and p.task == "sr" and not hasattr(p, "sr_filter")
    import settings
    a = settings.DefaultArgParser().parse_args(["--task", "sr", "--sr_factor", "2"])
    assert a.sr_kernel is None and a.sr_phase == 0
    assert type(physics.get_physics(a, "cpu")) is physics.Downsampling


def test_get_physics_builds_the_blur_the_deblurring_flags_would():
    import physics
    from physics._ops import BlurDecimateOp
    p = physics.get_physics(_args(sr_kernel="Gaussian_R1", sr_factor=4, sr_phase=3), "cpu")
    assert isinstance(p, physics.BlurDownsampling) and p.rate == 4 and p.phase == 3 and p.task == "sr"
    assert p.padding == "circular" and p.sr_filter.shape == (1, 1, 7, 7) and abs(p.noise_model.sigma - 5 / 255) < 1e-12
    assert isinstance(p._op, BlurDecimateOp) and p._op.route == "kernel" and p._op.shape == (7, 7)    # circular: the kernel
    # the names BM3D, the inverse filter and Noise2Inverse read must stay absent
    assert not hasattr(p, "filter") and not hasattr(p, "kernel")
    assert p.A_transpose == p.A_adjoint
    for padding in ("replicate", "reflect"):
        for v2 in (True, False):
            p = physics.get_physics(_args(sr_kernel="Gaussian_R1", blur_padding=padding, physics_v2=v2), "cpu")
            assert p.padding == padding and p._op.mode == padding and p._op.route == "bands" and p._op.pad == (3, 3)
    # the legacy circular rule puts a zero tap in front of an even axis, as Blur.__init__ does; BlurV2's does not
    k = rand_kernel(5, 4, 1)[None, None]
    legacy = physics.BlurDownsampling(filter=k, rate=2, padding="circular", v2=False)
    assert legacy._op.shape == (5, 5) and np.array_equal(legacy._op._host[:, 0], np.zeros(5))
    assert np.array_equal(legacy._op._host[:, 1:], k[0, 0].numpy())
    assert np.array_equal(legacy._op._host, physics.Blur(filter=k, padding="circular")._op._host[0])
    assert physics.BlurDownsampling(filter=k, rate=2, padding="circular", v2=True)._op.shape == (5, 4)
    assert physics.BlurDownsampling(filter=k, rate=2, padding="replicate")._op.route == "kernel"       # not rank 1


def test_flag_refusals_name_the_flag():
    import physics
    with pytest.raises(ValueError, match="--sr_kernel.*--task sr"):
        physics.get_physics(_args(task="deblurring", kernel="Gaussian_R2", sr_factor=None, sr_kernel="Gaussian_R1"), "cpu")
    with pytest.raises(ValueError, match="--sr_kernel.*--task sr"):
        physics.get_physics(_args(task="invert_a_tomography_like_filter", sr_kernel="Gaussian_R1"), "cpu")
    for phase in (2, 5, -1):
        with pytest.raises(ValueError, match="--sr_phase.*--sr_factor"):
            physics.get_physics(_args(sr_kernel="Gaussian_R1", sr_phase=phase), "cpu")
    with pytest.raises(ValueError, match="--sr_phase.*--sr_kernel"):
        physics.get_physics(_args(sr_phase=1), "cpu")
    with pytest.raises(ValueError, match="--sr_kernel.*--sr_factor"):
        physics.get_physics(_args(sr_kernel="Gaussian_R1", sr_factor=None), "cpu")
    with pytest.raises(ValueError, match="--blur_padding.*valid"):
        physics.get_physics(_args(sr_kernel="Gaussian_R1", blur_padding="valid"), "cpu")
    k = physics.get_kernel("Gaussian_R1")[None, None]
    with pytest.raises(ValueError, match="valid"):
        physics.BlurDownsampling(filter=k, rate=2, padding="valid")
    with pytest.raises(ValueError, match="padding"):
        physics.BlurDownsampling(filter=k, rate=2, padding="zero")
    with pytest.raises(ValueError, match="rate"):
        physics.BlurDownsampling(filter=k, rate=9)
    with pytest.raises(ValueError):                                   # per-channel colour filters
        physics.BlurDownsampling(filter=k.expand(1, 3, 7, 7), rate=2)
    op = physics.BlurDownsampling(filter=k, rate=2, padding="reflect")._op
    with pytest.raises(ValueError, match="7 taps.*extent of 3 "):
        op.check_extent(12, 3)
    op.check_extent(4, 4)


def test_parsers_take_the_flags():
    import settings
    import train
    a = train.build_parser().parse_args(["--task", "sr", "--sr_factor", "2", "--sr_kernel", "Gaussian_R1", "--sr_phase", "1",
                                         "--blur_padding", "reflect"])
    assert (a.sr_kernel, a.sr_phase, a.blur_padding) == ("Gaussian_R1", 1, "reflect")
    assert settings.DefaultArgParser().parse_args(["--sr_kernel", "k.pt"]).sr_kernel == "k.pt"
