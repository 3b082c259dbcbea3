"""The replicate, reflect and valid boundaries of physics.Blur on the host: the axis matrices of physics/_bands against the
reference's own outputs (G19) and a brute-force loop, the refusals, the --blur_padding flag, and the argument checks of
sei_blur_dense_pad (made before any HIP call, so they run without a GPU)."""
import argparse

import numpy as np
import pytest
import torch

PADDINGS = ("valid", "circular", "replicate", "reflect")
G19_KERNELS = ("rand5x5", "rand4x6", "rand1x7", "rand3x1", "Gaussian_R1", "Box_R2")
SEPARABLE = ("Gaussian_R1", "Box_R2")
TOL = 2e-6           # max-norm, relative to the fixture's max-abs


def g19(golden):
    return golden("g19_blur_paddings")


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def brute_axis_matrix(n, taps, mode):
    """The rule of the axis, written out again: the image padded by p explicitly, then a sliding window over it."""
    K = len(taps)
    s, p = {1: (0, 1)}.get(K, (K // 2, K // 2) if K % 2 else (K // 2 - 1, K // 2))
    if mode == "circular":
        src = [(j - p) % n for j in range(n + 2 * p)]
    elif mode == "replicate":
        src = [0] * p + list(range(n)) + [n - 1] * p
    elif mode == "reflect":
        src = list(range(p, 0, -1)) + list(range(n)) + list(range(n - 2, n - 2 - p, -1))
    else:
        src = None
    rows = n - 2 * p if mode == "valid" else n
    m = np.zeros((rows, n), dtype=np.float64)
    for i in range(rows):
        for a in range(K):
            j = i - a + s + p                       # position in the padded image (valid: i' + p - a + s in the image)
            m[i, j if src is None else src[j]] += float(taps[a])
    return m


def test_fixture_holds_every_case(golden):
    g = g19(golden)
    assert g["x"].shape == (2, 3, 17, 21) and g["x"].dtype == np.float32
    shapes = {"rand5x5": (5, 5), "rand4x6": (4, 6), "rand1x7": (1, 7), "rand3x1": (3, 1), "Gaussian_R1": (7, 7),
              "Box_R2": (5, 5)}
    for name in G19_KERNELS:
        k = g[f"k.{name}"]
        assert k.shape == shapes[name] and abs(k.sum() - 1) < 1e-6
        if name not in SEPARABLE and min(k.shape) > 1:
            assert np.linalg.matrix_rank(k) > 1
        for padding in PADDINGS:
            y, ct, adj = (g[f"{name}.{padding}.{what}"] for what in ("y", "g", "adj"))
            assert y.dtype == ct.dtype == adj.dtype == np.float32
            assert ct.shape == y.shape and adj.shape == g["x"].shape
            if padding != "valid":
                assert y.shape == g["x"].shape


def test_offsets_table():
    from physics import _bands
    assert _bands.blur_axis_offsets(1) == (0, 1)
    assert _bands.blur_axis_offsets(4) == (1, 2)
    assert _bands.blur_axis_offsets(5) == (2, 2)
    # a 1-wide axis shrinks by 2 in valid, as in the reference
    assert _bands.blur_axis_matrix(9, [1.0], "valid").shape == (7, 9)
    assert np.array_equal(_bands.blur_axis_matrix(9, [1.0], "valid"), np.eye(9)[1:8])


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("name", SEPARABLE)
def test_axis_matrices_vs_reference(golden, name, padding):
    """M_v x M_h^T and M_v^T g M_h in float64 against the reference's conv / conv_transpose."""
    from physics import _bands
    g = g19(golden)
    k = g[f"k.{name}"]
    tv, th = k.sum(1) / k.sum(), k.sum(0)
    mv, mh = _bands.blur_axis_matrix(17, tv, padding), _bands.blur_axis_matrix(21, th, padding)
    x, ct = g["x"].astype(np.float64), g[f"{name}.{padding}.g"].astype(np.float64)
    e_fwd = relerr(mv @ x @ mh.T, g[f"{name}.{padding}.y"])
    e_adj = relerr(mv.T @ ct @ mh, g[f"{name}.{padding}.adj"])
    print(f"{name} {padding}: forward {e_fwd:.2e} adjoint {e_adj:.2e}")
    assert e_fwd < TOL and e_adj < TOL, (name, padding, e_fwd, e_adj)


@pytest.mark.parametrize("padding", ["circular", "replicate", "reflect"])
@pytest.mark.parametrize("n", [5, 6, 4])
def test_end_rows_when_the_extent_is_within_twice_the_padding(n, padding):
    """Seven taps (p = 3) on 5 and 6 pixels: every row is an end row, and rows near one end reach past the other. n = 4
    is the smallest extent reflect takes (p = n - 1)."""
    from physics import _bands
    taps = np.random.default_rng(7).random(7)
    got = _bands.blur_axis_matrix(n, taps, padding)
    want = brute_axis_matrix(n, taps, padding)
    assert got.dtype == np.float64 and got.shape == (n, n) and np.abs(got - want).max() < 1e-15
    assert np.abs(got.sum(1) - taps.sum()).max() < 1e-14            # every row holds every tap once


@pytest.mark.parametrize("K", [1, 4, 5])
def test_every_mode_vs_brute_force(K):
    from physics import _bands
    taps = np.random.default_rng(K).random(K)
    for padding in PADDINGS:
        assert np.abs(_bands.blur_axis_matrix(11, taps, padding) - brute_axis_matrix(11, taps, padding)).max() < 1e-15


def test_unknown_paddings_are_refused():
    import physics
    k = physics.get_kernel("Gaussian_R1")[None, None]
    for padding in ("zero", "constant", "zeros", None):
        with pytest.raises(ValueError, match="padding"):
            physics.Blur(filter=k, padding=padding)
    with pytest.raises(ValueError):                                   # per-channel colour filters
        physics.Blur(filter=k.expand(1, 3, 7, 7), padding="replicate")
    from physics import _bands
    with pytest.raises(ValueError, match="padding"):
        _bands.blur_axis_matrix(9, [0.5, 0.5], "zero")
    from physics._ops import PaddedBlurOp
    with pytest.raises(ValueError, match="padding"):
        PaddedBlurOp(k, "circular")                                   # CircularBlurOp is the circular route


def test_reflect_beyond_the_extent_is_refused_by_name():
    import physics
    from physics import _bands
    with pytest.raises(ValueError, match="extent of 3 "):
        _bands.blur_axis_matrix(3, np.ones(7) / 7, "reflect")          # p = 3 > n - 1 = 2
    assert _bands.blur_axis_matrix(4, np.ones(7) / 7, "reflect").shape == (4, 4)
    op = physics.Blur(filter=physics.get_kernel("Gaussian_R1")[None, None], padding="reflect")._op      # 7 x 7
    with pytest.raises(ValueError) as err:
        op.check_extent(12, 3)
    assert "extent of 3" in str(err.value) and "7 taps" in str(err.value) and "12x3" in str(err.value)
    op.check_extent(4, 4)
    with pytest.raises(ValueError, match="valid"):
        _bands.blur_axis_matrix(6, np.ones(7) / 7, "valid")           # n <= 2p
    valid = physics.Blur(filter=physics.get_kernel("Gaussian_R1")[None, None], padding="valid")._op
    with pytest.raises(ValueError, match="extent above 6"):
        valid.check_extent(6, 9)
    valid.check_extent(7, 7)


def test_rank_one_test_matches_the_circular_operator(golden):
    from physics._ops import CircularBlurOp, PaddedBlurOp
    g = g19(golden)
    for name in G19_KERNELS:
        k = torch.from_numpy(g[f"k.{name}"])
        assert PaddedBlurOp(k, "replicate").separable == CircularBlurOp(k).separable
        assert PaddedBlurOp(k, "replicate").separable == (name in SEPARABLE or min(k.shape) == 1)


def _args(**over):
    base = dict(task="deblurring", kernel="Gaussian_R2", sr_factor=None, noise_level=5, physics_v2=True,
                physics_true_adjoint=False)
    base.update(over)
    return argparse.Namespace(**base)


def test_get_physics_honours_and_defaults_the_flag():
    import physics
    p = physics.get_physics(_args(), "cpu")                                  # a bare namespace: no flag at all
    assert isinstance(p, physics.BlurV2)
    p = physics.get_physics(_args(blur_padding="circular"), "cpu")
    assert isinstance(p, physics.BlurV2)
    p = physics.get_physics(_args(blur_padding="circular", physics_v2=False), "cpu")
    assert isinstance(p, physics.Blur) and p.padding == "circular"
    for v2 in (True, False):                                                 # the FFT operator has no other boundary
        for padding in ("replicate", "reflect"):
            p = physics.get_physics(_args(blur_padding=padding, physics_v2=v2), "cpu")
            assert isinstance(p, physics.Blur) and p.padding == padding and p._op.mode == padding
            assert p._op.separable and p.task == "deblurring" and p.filter.shape == (1, 1, 13, 13)
            assert abs(p.noise_model.sigma - 5 / 255) < 1e-12
    # other tasks ignore it
    assert isinstance(physics.get_physics(_args(task="sr", sr_factor=2, kernel=None, blur_padding="reflect"), "cpu"),
                      physics.Downsampling)


def test_parser_takes_three_paddings_and_refuses_valid(capsys):
    import settings
    import train
    assert settings.DefaultArgParser().parse_args([]).blur_padding == "circular"
    for padding in ("circular", "replicate", "reflect"):
        assert settings.DefaultArgParser().parse_args(["--blur_padding", padding]).blur_padding == padding
    assert train.build_parser().parse_args(["--blur_padding", "reflect"]).blur_padding == "reflect"
    for bad in ("valid", "zero"):
        with pytest.raises(SystemExit):
            settings.DefaultArgParser().parse_args(["--blur_padding", bad])
        assert "--blur_padding" in capsys.readouterr().err


# Fake device pointers for calls that must be refused: never dereferenced, because a refused call launches nothing.
X, Y, K_, WORK = 1 << 20, 2 << 20, 3 << 20, 4 << 20
BAD_ARG, TOO_LARGE = 10001, 10002


def test_entry_point_refuses_bad_arguments_on_the_host():
    import _native
    L = _native.lib()

    def call(x=X, y=Y, k=K_, kv=5, kh=5, planes=2, H=17, W=21, mode=1, transpose=0, work=WORK):
        return L.sei_blur_dense_pad(x, y, k, kv, kh, planes, H, W, mode, transpose, work, None)

    def query(planes=2, H=17, W=21, kv=5, kh=5, mode=1, transpose=1):
        return L.sei_blur_dense_pad_work_floats(planes, H, W, kv, kh, mode, transpose)

    for null in ("x", "y", "k"):
        assert call(**{null: None}) == BAD_ARG
    assert call(transpose=1, work=None) == BAD_ARG                  # the adjoint's canvas is required ...
    assert query() == 2 * (17 + 4) * (21 + 4)
    assert query(transpose=0) == 0 and query(mode=3) == 0          # ... only there
    assert query(kv=4, kh=1) == 2 * (17 + 4) * (21 + 2)             # p = (2, 1)
    for mode in (0, 4, -1):                                         # 0: the circular entry point is the circular route
        assert call(mode=mode) == BAD_ARG and call(mode=mode, transpose=1) == BAD_ARG
        assert query(mode=mode) == 0
    for taps in (dict(kv=64), dict(kh=64), dict(kv=64, kh=64)):
        assert call(**taps) == TOO_LARGE and call(transpose=1, **taps) == TOO_LARGE
        assert query(**taps) == 0
    for size in (dict(planes=0), dict(H=0), dict(W=-1), dict(kv=0), dict(kh=0)):
        assert call(**size) == BAD_ARG and query(**size) == 0
    # reflect needs p <= n - 1, valid n > 2p
    assert call(mode=2, kv=7, H=3) == BAD_ARG and query(mode=2, kv=7, H=3) == 0
    assert query(mode=2, kv=7, H=4) == 2 * (4 + 6) * (21 + 4)
    assert call(mode=3, kh=7, W=6) == BAD_ARG and call(mode=3, kh=7, W=6, transpose=1) == BAD_ARG
    # overlapping operands
    n = 2 * 17 * 21 * 4
    assert call(y=X) == BAD_ARG and call(y=X + n - 4) == BAD_ARG and call(y=X - n + 4) == BAD_ARG
    assert call(k=Y + 8) == BAD_ARG
    assert call(transpose=1, work=X + 64) == BAD_ARG and call(transpose=1, work=Y - 16) == BAD_ARG
    assert call(transpose=1, work=K_ - 4) == BAD_ARG
