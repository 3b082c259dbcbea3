"""CPU: the noise estimator's restatement (tests/noise_est_ref.py) at its own edge cases and on a synthetic measurement, the
two entry points' host-side refusals, and the flags of the two drivers.

The statistical bounds are conditions set before any code ran (sigma within 5 %; for Poisson-Gaussian noise the variance at
signal 0.5 within 10 % and the gain within 25 %), on 3 x 256 x 256 piecewise-constant rectangles plus low-frequency
sinusoids, circularly blurred with a Gaussian of standard deviation 1.5. Printed by these tests on the restatement (float
measurement / 8-bit quantised):

  Gaussian 5 / 255                  sigma +0.41 % / +0.51 %   (the quantised figure includes the 1/12 LSB^2 of rounding)
  Gaussian 10 / 255                 sigma +0.03 % / +0.05 %
  Poisson-Gaussian (2/255, 0.01)    variance at 0.5 -0.53 % / -0.45 %, gain -5.30 % / -5.26 %
  Poisson-Gaussian (5/255, 0.003)   variance at 0.5 -0.36 % / -0.78 %, gain -1.47 % / -2.00 %
"""
import math

import numpy as np
import pytest

import noise_est_ref as R


# ------------------------------------------------------------------------------------------------ hand-built histograms
def empty():
    return np.zeros((R.LEVELS, R.BINS), dtype=np.uint64)


def level_row(hist, level, median_bin, count):
    """`count` quads at `level` whose interpolated median lies in `median_bin`: a quarter below, half in it, a quarter above
    (all in it for bin 0)."""
    if median_bin == 0:
        hist[level, 0] += count
        return
    hist[level, median_bin - 1] += count // 4
    hist[level, median_bin] += count // 2
    hist[level, median_bin + 1] += count - count // 4 - count // 2


def edge_histograms():
    """name -> (histogram, expected flags); shared with the GPU file, which runs sei_noise_fit on the same histograms."""
    cases = {}
    cases["empty"] = (empty(), R.FLAG_EMPTY)
    h = empty()
    h[20, 3] = 1
    cases["single quad"] = (h, R.FLAG_NO_LINE)
    h = empty()
    h[30, 0] = 1000
    h[31, 0] = 1000
    cases["median in bin 0"] = (h, 0)                         # equal v on two levels: a line of slope 0, nothing clamped
    h = empty()
    h[30, 255] = 600
    h[30, 7] = 300
    cases["median in the overflow bin"] = (h, R.FLAG_POOLED_OVERFLOW | R.FLAG_NO_LINE)
    h = empty()
    for level, b in ((10, 12), (25, 10), (40, 8), (55, 6)):
        level_row(h, level, b, 4000)
    cases["negative slope"] = (h, R.FLAG_NEGATIVE_SLOPE)
    h = empty()
    for level, b in ((30, 2), (40, 10), (50, 20)):
        level_row(h, level, b, 4000)
    cases["negative intercept"] = (h, R.FLAG_NEGATIVE_INTERCEPT)
    h = empty()
    level_row(h, 30, 9, 4000)
    level_row(h, 3, 9, 4000)                                  # below LEVEL_LO
    level_row(h, 60, 9, 4000)                                 # above LEVEL_HI
    level_row(h, 40, 9, 200)                                  # fewer than N_MIN quads
    cases["one usable level"] = (h, R.FLAG_NO_LINE)
    h = empty()
    for level, b in ((10, 8), (20, 9), (30, 10), (45, 11), (57, 12)):
        level_row(h, level, b, 5000 + 37 * level)
    cases["a clean line"] = (h, 0)
    return cases


EDGES = edge_histograms()


@pytest.mark.parametrize("name", sorted(EDGES))
def test_ref_flags_of_the_edge_histograms(name):
    hist, flags = EDGES[name]
    out = R.fit(hist)
    assert int(out[5]) == flags and out[4] == float(hist.sum()) and out[6:] == [0.0, 0.0]


def test_ref_single_quad():
    hist = R.quad_hist(np.array([[[0.5, 0.25], [0.25, 0.75]]], dtype=np.float32))
    # s = 0.4375 -> level 28; t = (0.25 - (-0.5)) / 2 = 0.375 -> floor(191.25 + 0.5) = 191
    assert hist.sum() == 1 and hist[28, 191] == 1
    sigma, eta, gamma, used, quads, flags = R.fit(hist)[:6]
    # half = 0.5 of the one count in bin 191: the median is the bin's centre
    assert sigma == pytest.approx(191 / 510 / R.C_MAD, rel=1e-15)
    assert (eta, gamma, used, quads, flags) == (sigma * sigma, 0.0, 0.0, 1.0, R.FLAG_NO_LINE)


def test_ref_empty_histogram():
    # clipped and non-finite pixels leave nothing to count
    y = np.array([[[0.0, 0.5], [0.5, 0.5]], [[1.0, 0.5], [0.5, 0.5]], [[np.nan, 0.5], [0.5, 0.5]],
                  [[0.5, np.inf], [0.5, 0.5]], [[0.5, 0.5], [-0.1, 0.5]], [[0.5, 0.5], [0.5, 1.2]]], dtype=np.float32)
    hist = R.quad_hist(y)
    assert hist.sum() == 0
    out = R.fit(hist)
    assert all(math.isnan(v) for v in out[:3]) and out[3:] == [0.0, 0.0, 1.0, 0.0, 0.0]


def test_ref_median_in_bin_0_is_half_a_bin():
    sigma, eta, gamma, used, _, flags = R.fit(EDGES["median in bin 0"][0])[:6]
    # bin 0 is [0, 0.5) on the lattice; half the counts in: the median is its middle
    assert sigma == pytest.approx(0.25 / 510 / R.C_MAD, rel=1e-15) and used == 2.0
    assert (gamma, eta) == (0.0, sigma * sigma)


def test_ref_median_in_the_overflow_bin():
    sigma, eta, gamma, used, quads, _ = R.fit(EDGES["median in the overflow bin"][0])[:6]
    assert math.isnan(sigma) and math.isnan(eta) and gamma == 0.0 and used == 0.0 and quads == 900.0


def test_ref_clamps():
    sigma, eta, gamma, used, _, _ = R.fit(EDGES["negative slope"][0])[:6]
    medians = [R.median(EDGES["negative slope"][0][l])[0] / R.C_MAD for l in (10, 25, 40, 55)]
    assert gamma == 0.0 and used == 4.0 and eta == pytest.approx(np.mean([q * q for q in medians]), rel=1e-14)
    sigma, eta, gamma, used, _, _ = R.fit(EDGES["negative intercept"][0])[:6]
    ms = [(l + 0.5) / 64 for l in (30, 40, 50)]
    vs = [(R.median(EDGES["negative intercept"][0][l])[0] / R.C_MAD) ** 2 for l in (30, 40, 50)]
    assert eta == 0.0 and used == 3.0
    assert gamma == pytest.approx(sum(m * v for m, v in zip(ms, vs)) / sum(m * m for m in ms), rel=1e-14)
    sigma, eta, gamma, used, _, _ = R.fit(EDGES["one usable level"][0])[:6]
    assert used == 1.0 and gamma == 0.0 and eta == sigma * sigma


def test_ref_line_against_numpy_polyfit():
    hist = EDGES["a clean line"][0]
    sigma, eta, gamma, used, _, flags = R.fit(hist)[:6]
    levels = (10, 20, 30, 45, 57)
    m = np.array([(l + 0.5) / 64 for l in levels])
    v = np.array([(R.median(hist[l])[0] / R.C_MAD) ** 2 for l in levels])
    w = np.array([float(hist[l].sum()) for l in levels])
    slope, intercept = np.polyfit(m, v, 1, w=np.sqrt(w))
    assert used == 5.0 and flags == 0
    assert gamma == pytest.approx(slope, rel=1e-9) and eta == pytest.approx(intercept, rel=1e-9)


def test_ref_histogram_rules():
    """Odd extents drop the trailing row and column; ties of the 8-bit lattice sit at bin centres; the level boundary l / 64
    belongs to level l; exact 0 and 1 drop the quad."""
    y = np.full((1, 3, 5), 0.5, dtype=np.float32)
    y[0, 2, :] = np.nan                                      # the trailing row is never read into a quad
    y[0, :, 4] = np.nan
    hist = R.quad_hist(y)
    assert hist.sum() == 2 and hist[32, 0] == 2              # s = 0.5 exactly: level 32
    n = np.float32(1) / np.float32(255)
    quad = np.array([[[100 * n, 100 * n], [100 * n, 103 * n]]], dtype=np.float32)       # t = 1.5 / 255: bin 3
    hist = R.quad_hist(quad)
    assert hist.sum() == 1 and hist[:, 3].sum() == 1
    assert R.quad_hist(np.array([[[0.5, 0.5], [0.5, 1.0]]], dtype=np.float32)).sum() == 0


# ------------------------------------------------------------------------------------------------ statistical sanity
@pytest.fixture(scope="module")
def blurred():
    return R.circular_blur(R.clean_image())


@pytest.mark.parametrize("quantise", [False, True])
@pytest.mark.parametrize("sigma", R.GAUSSIAN_CASES)
def test_ref_gaussian_level(blurred, sigma, quantise):
    R.hold_gaussian(f"restatement, quantised {quantise}", R.estimate(R.measure(blurred, sigma, 0, 1, quantise)), sigma)


@pytest.mark.parametrize("quantise", [False, True])
@pytest.mark.parametrize("sigma,gain", R.PG_CASES)
def test_ref_poisson_gaussian_levels(blurred, sigma, gain, quantise):
    est = R.estimate(R.measure(blurred, sigma, gain, 2, quantise))
    R.hold_poisson_gaussian(f"restatement, quantised {quantise}", est, sigma, gain)
    assert int(est[5]) == 0 and est[3] >= 40


# ------------------------------------------------------------------------------------------------ the C ABI, no GPU needed
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    import _native
    L = _native.lib()
    P = 4096                                                 # a fake device pointer: a refused call launches nothing
    assert L.sei_noise_quad_hist(None, 3, 8, 8, P, 0, None) == 10001
    assert L.sei_noise_quad_hist(P, 3, 8, 8, None, 0, None) == 10001
    for bad in ((0, 8, 8), (-1, 8, 8), (3, 1, 8), (3, 8, 1), (3, 0, 8), (3, 8, 0), (1, 1 << 15, 1 << 15)):
        assert L.sei_noise_quad_hist(P, *bad, 2 * P, 0, None) == 10001, bad
    assert L.sei_noise_fit(None, P, None) == 10001
    assert L.sei_noise_fit(P, None, None) == 10001
    assert _native.SIGNATURES["sei_noise_fit"] == [_native._P] * 3 and len(_native.SIGNATURES["sei_noise_quad_hist"]) == 7
    assert L.sei_abi_version() == 12


def test_host_layer_refuses_cpu_tensors():
    import torch
    import _native
    import noise_estimation
    with pytest.raises(_native.NativeLibraryError):
        noise_estimation.estimate_noise(torch.rand(3, 16, 16))
    with pytest.raises(_native.NativeLibraryError):
        noise_estimation.NoiseEstimator("cpu")


# ------------------------------------------------------------------------------------------------ the drivers' flags
FLAG = "--unsure_init_from_measurements"
COMMON = ["--device", "cuda", "--task", "deblurring", "--kernel", "Gaussian_R2", "--out_dir", "unused", "--method", "proposed",
          "--fine_tuning"]


def test_train_py_refuses_the_flag_by_name(tmp_path):
    """train.main stops in front of get_physics: nothing here touches a GPU."""
    import train
    folder = str(tmp_path)
    with pytest.raises(ValueError, match=f"{FLAG}.*--sure_unknown_noise"):
        train.main(COMMON + ["--dataset", folder, FLAG])
    with pytest.raises(ValueError, match=f"{FLAG}.*folder"):
        train.main(COMMON[:-1] + ["--dataset", "synthetic", "--sure_unknown_noise", FLAG])
    with pytest.raises(ValueError, match=f"{FLAG}.*--unsure_init_noise_level"):
        train.main(COMMON + ["--dataset", folder, "--sure_unknown_noise", FLAG, "--unsure_init_noise_level", "12"])
    with pytest.raises(ValueError, match=f"{FLAG}.*--unsure_init_gain"):
        train.main(COMMON + ["--dataset", folder, "--sure_unknown_noise", "--unsure_noise_model", "poisson_gaussian", FLAG,
                             "--unsure_init_gain", "0.01"])
    args = train.build_parser().parse_args(COMMON)
    assert args.unsure_init_from_measurements is False
    train.check_unsure_init_args(args)                       # off: nothing is looked at
    args = train.build_parser().parse_args(COMMON + ["--dataset", folder, "--sure_unknown_noise", FLAG])
    train.check_unsure_init_args(args)                       # accepted


def test_test_py_knows_estimate_noise(capsys):
    from test_bootstrap import load_test_py
    test_py = load_test_py()
    assert test_py.parse_args(["--task", "deblurring"]).estimate_noise is None
    for kind in ("gaussian", "poisson_gaussian"):
        assert test_py.parse_args(["--task", "deblurring", "--estimate_noise", kind]).estimate_noise == kind
    with pytest.raises(SystemExit):
        test_py.parse_args(["--task", "deblurring", "--estimate_noise", "laplace"])
    assert "--estimate_noise" in capsys.readouterr().err
