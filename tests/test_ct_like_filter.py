"""CTLikeFilter without a GPU: the circulant form (physics/_circulant.py) against the reference's own outputs (G16:
tests/golden/g16_ct_like_filter*.npz, written by tools/gen_golden.py from src/physics/ct_like_filter.py), the host-side
argument checks of sei_circ_filter_sep, and get_loss on the task's missing default margin."""
import argparse

import numpy as np
import pytest

TOL = 1e-11          # float64 against float64, the bar of tests/test_oracle_golden.py
G16 = ("g16_ct_like_filter", "g16_ct_like_filter_big_a", "g16_ct_like_filter_big_b")
TAGS = {"sq": (2, 3, 48, 48), "rect": (1, 3, 47, 33), "tiny": (1, 1, 1, 5), "odd": (1, 1, 19, 23), "big": (1, 1, 256, 256)}


def g16(golden):
    out = {}
    for name in G16:
        f = golden(name)
        out.update({k: f[k] for k in f.files})
    return out


def rel(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / np.abs(b).max())


def apply2(v, inverse, dims=(2, 3)):
    """C_H v C_W^T on the last two axes with physics._circulant.dense (identity on an axis not in `dims`), float64."""
    from physics import _circulant
    v = np.asarray(v, dtype=np.float64)
    if 2 in dims:
        v = np.einsum("ir,bcrw->bciw", _circulant.dense(v.shape[2], inverse), v)
    if 3 in dims:
        v = np.einsum("wj,bcij->bciw", _circulant.dense(v.shape[3], inverse), v)
    return v


@pytest.mark.parametrize("tag", list(TAGS))
def test_dense_circulant_reproduces_the_reference(golden, tag):
    g = g16(golden)
    x = g[f"{tag}.f32.x"]
    assert x.shape == TAGS[tag] and x.dtype == np.float32
    assert rel(apply2(x, True), g[f"{tag}.f64.A"]) < TOL
    assert rel(apply2(x, False), g[f"{tag}.f64.Adag"]) < TOL
    if tag == "big":
        return
    ct = g[f"{tag}.f32.ct"]
    assert rel(apply2(ct, True), g[f"{tag}.f64.gA"]) < TOL            # the vjp of A is A: symmetric
    assert rel(apply2(ct, False), g[f"{tag}.f64.gAdag"]) < TOL
    if tag in ("rect", "odd"):
        assert rel(apply2(x, True, dims=(2,)), g[f"{tag}.f64.f1d_dim2_inv"]) < TOL
        assert rel(apply2(x, False, dims=(3,)), g[f"{tag}.f64.f1d_dim3_fwd"]) < TOL


@pytest.mark.parametrize("n", [1, 2, 5, 48, 255, 256])
def test_the_two_circulants_are_symmetric_inverses(n):
    from physics import _circulant
    a, d = _circulant.dense(n, True), _circulant.dense(n, False)
    assert a.shape == (n, n) and a.dtype == np.float64
    assert np.abs(a @ d - np.eye(n)).max() < TOL
    assert np.abs(a - a.T).max() < TOL * np.abs(a).max() and np.abs(d - d.T).max() < TOL * np.abs(d).max()
    assert np.array_equal(_circulant.first_column(n, True), a[:, 0])
    with pytest.raises(ValueError):
        _circulant.first_column(0, True)


def test_entry_point_checks_its_arguments_on_the_host():
    import _native
    assert len(_native.SIGNATURES["sei_circ_filter_sep"]) == 8
    L = _native.lib()
    assert L.sei_circ_filter_sep(None, None, None, None, 1, 8, 8, None) == 10001
    assert L.sei_circ_filter_sep(16, 16, 32, 48, 1, 8, 8, None) == 10001            # x == y
    for planes, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        assert L.sei_circ_filter_sep(16, 32, 48, 64, planes, H, W, None) == 10001
    # beyond the LDS budget of a workgroup: refused, never launched (512 x 512 itself is inside, tested on the GPU)
    assert L.sei_circ_filter_sep(16, 32, 48, 64, 1, 2048, 2048, None) == 10002
    assert L.sei_circ_filter_sep(16, 32, 48, 64, 1, 1 << 20, 8, None) == 10002


def test_the_task_builds_its_physics_and_needs_an_explicit_margin():
    import physics
    from losses import get_loss
    args = argparse.Namespace(task="invert_a_tomography_like_filter", kernel=None, sr_factor=None, noise_level=5,
                              physics_v2=True, physics_true_adjoint=False)
    p = physics.get_physics(args, device="cpu")                  # building it touches no device
    assert isinstance(p, physics.CTLikeFilter) and p.task == args.task and p.eps == 1
    assert not hasattr(p, "rate") and not hasattr(p, "filter")

    class Stub:
        task = args.task
    with pytest.raises(ValueError, match="--sure_margin.*--no-partial_sure"):
        get_loss(argparse.Namespace(task=args.task, partial_sure=True, sure_margin=None, partial_sure_sr=False), Stub())
