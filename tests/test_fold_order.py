"""CPU tests of oracle/fold_order.py, the numpy model of the order in which csrc/reduce_kernels.hip folds partial sums
(tests/test_fold_order_gpu.py holds the kernels to the model bit for bit; here the model is held to the sums it claims)."""
import numpy as np
import pytest

from oracle import fold_order as fo

GROUPS = (1, 15, 16, 17, 49, 63, 64, 65, 129, 300, 1024)      # every turn of the slice loop: empty slices, tail only, main + tail


@pytest.mark.parametrize("groups", GROUPS)
def test_fold_model_is_exact_on_integers(groups):
    """Integer-valued partial sums add without rounding in any order: the model must visit every group exactly once."""
    rng = np.random.default_rng(groups)
    part = rng.integers(-8, 9, size=(groups, 72)).astype(np.float32)
    assert np.array_equal(fo.fold_segment(part), part.sum(0, dtype=np.float64).astype(np.float32))


@pytest.mark.parametrize("groups", GROUPS)
def test_fold_model_is_a_float32_sum(groups):
    """Random data: within the bound of that many float32 additions, (n - 1) u sum|p| with u = 2^-24 (Higham, Accuracy and
    Stability of Numerical Algorithms, 4.2) -- a column meets at most groups + 16 of them -- of the float64 sum."""
    rng = np.random.default_rng(1000 + groups)
    part = rng.standard_normal((groups, 72)).astype(np.float32)
    err = np.abs(fo.fold_segment(part).astype(np.float64) - part.astype(np.float64).sum(0))
    assert np.all(err <= (groups + 16) * 2.0 ** -24 * np.abs(part).astype(np.float64).sum(0))


def test_fold_model_destinations():
    """Both destination mappings on a hand-built case: entry e = C t + c of the depthwise layout holds the value
    1000 t + c, so gw[c][t] and gbias[c] show where each entry went; the split layout a | b | c with c dropped or kept;
    two segments on a running value."""
    C = 3
    row = np.array([1000 * t + c for t in range(50) for c in range(C)], np.float32)
    part = np.stack([row, 2 * row])                                          # two groups: entry sums 3 * (1000 t + c)
    gw0, gb0 = np.full((C, 49), 0.5, np.float32), np.full(C, 0.25, np.float32)
    gw, gb, _ = fo.fold_job(fo.FOLD_DWCONV7, C, [part], gw0, gb0)
    for c in range(C):
        for t in range(49):
            assert gw[c, t] == 0.5 + 3 * (1000 * t + c)
        assert gb[c] == 0.25 + 3 * (49000 + c)
    gw2, gb2, _ = fo.fold_job(fo.FOLD_DWCONV7, C, [part], gw0, None)          # no bias gradient wanted
    assert gb2 is None and np.array_equal(gw2, gw)
    assert np.all(gw0 == 0.5) and np.all(gb0 == 0.25)                        # the inputs are left alone

    split = 4
    seg1 = np.arange(2 * 12, dtype=np.float32).reshape(2, 12)                # column sums 12 + 2 e
    seg2 = np.ones((17, 12), np.float32)                                     # + 17
    want = 12 + 2 * np.arange(12, dtype=np.float32) + 17
    a, b, c = fo.fold_job(fo.FOLD_SPLIT, split, [seg1, seg2], np.full(split, 100, np.float32), np.full(split, 200, np.float32),
                          np.full(split, 300, np.float32))
    assert np.array_equal(a, 100 + want[:4]) and np.array_equal(b, 200 + want[4:8]) and np.array_equal(c, 300 + want[8:])
    a2, b2, c2 = fo.fold_job(fo.FOLD_SPLIT, split, [seg1, seg2], np.full(split, 100, np.float32), np.full(split, 200, np.float32))
    assert np.array_equal(a2, a) and np.array_equal(b2, b) and c2 is None    # the third sum is dropped
    (cs, _, _) = fo.fold_job(fo.FOLD_SPLIT, split, [seg1[:, :4]], np.zeros(split, np.float32))   # a plain column sum
    assert np.array_equal(cs, want[:4] - 17)
