"""GPU: the BM3D kernels (sei_bm3d_match, sei_bm3d_ht, sei_bm3d_wiener, sei_bm3d_finish through models.bm3d) and the BM3D
baseline against the float64 restatement tests/bm3d_ref.py: the centring of the transfer function against the project's own
blur operators, matching (distances, positions, counts, determinism, batch independence), the two filters on injected groups,
the chain of the four steps each fed the restatement's previous output, the whole forward, and test.py end to end.

Bounds.
- DIST_REL = 70 * 2^-24: a distance is 64 squared differences of float32 values summed in float32 and scaled by a power of
  two: one rounding per difference, one per square, at most 63 of the sum, (1 + u)^66 - 1 < 70 u relative to the sum of the
  (non-negative) terms, which is the distance itself. Two distances can change order only if their relative gap is within
  2 DIST_REL (tau, rounded to float32, adds one more u, covered by the slack from 66 to 70): such reference blocks are
  excused, at most 2 % of a case.
- COEF_ERR and OUT_TOL are measured, as twice the largest figure observed over the cases of this file (the summation orders
  of the kernel and of the restatement legitimately differ): COEF_ERR is |kernel coefficient - float64 coefficient| /
  threshold over the coefficients with |c| < 2 threshold (a coefficient further away is not near a decision, whatever its
  error), OUT_TOL the largest |kernel output - float64 output| of the Wiener stage and of the hard-thresholding stage
  outside excused pixels, for planes in [0, 1]. Measured on an MI355X: coefficient error 1.013e-13 of the threshold at most
  (48 x 40 x 6, n_max 16: the hard-thresholding kernel transforms in double, so this is float64 rounding on both sides and
  no pixel of any case is excused), output error 1.166e-06 at most (Wiener, 48 x 40, n_max 32, agg 1; hard thresholding
  1.086e-06; lambd = 0 9.537e-07). Hence COEF_ERR = 2.026e-13 and OUT_TOL = 2.332e-06. Every test prints its figures before
  it asserts.
- INVERSE_TOL = 2^-22 of the largest value: the two inversions and the variances are computed in float64 on the device
  (errors of 1e-14 even after the inverse's gain of about 30) and then rounded to float32, half an ulp of each value, at
  most 2^-24 of the largest; the factor 4 is slack for the restatement's own float64 FFT.
- E2E_RMS: decisions may legitimately diverge end to end, so the bound is twice the largest RMS difference of the restatement
  in float32 against itself in float64 over the seeds of the test (tests/test_bm3d_baseline_gpu.py::e2e_case builds the
  inputs): measured on the CPU, never from the code under test.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bm3d_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
DIST_REL = 70 * 2.0 ** -24
COEF_ERR = 2 * 1.013e-13        # twice the largest observed (see the module docstring); measured figures are printed
OUT_TOL = 2 * 1.166e-6
INVERSE_TOL = 2.0 ** -22
E2E_SEEDS = (1, 2, 3)
E2E_RMS = 2 * 2.516e-5         # twice the largest float32-against-float64 RMS of the restatement over E2E_SEEDS
EXTENTS = ((8, 8), (16, 16), (21, 35), (48, 40))
SIGMA = 5 / 255


def planes_of(H, W, planes, seed, noise=0.02):
    """Smooth-plus-noise planes in [0, 1], float32 values held as float64 (planes, H, W)."""
    rng = np.random.default_rng(1000 + seed)
    x = R.smooth_image(H, W, seed, planes) + noise * rng.standard_normal((planes, H, W))
    return np.clip(x, 0, 1).astype(np.float32).astype(np.float64)


def on_gpu(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def batch_view(x, offset_view):
    """(6, H, W) float64 -> a (2, 3, H, W) float32 GPU batch; with offset_view a contiguous view 4 bytes into a buffer."""
    t = on_gpu(x).reshape(2, 3, *x.shape[-2:])
    if not offset_view:
        return t
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


_MATCH_CACHE = {}


def matched(H, W, planes, tau, n_max, seed=0):
    """The restatement's groups of a case, computed once: (x, [match_ref tuple per plane])."""
    key = (H, W, planes, tau, n_max, seed)
    if key not in _MATCH_CACHE:
        x = planes_of(H, W, planes, seed)
        _MATCH_CACHE[key] = (x, [R.match_ref(x[p], tau, n_max) for p in range(planes)])
    return _MATCH_CACHE[key]


def groups_on_gpu(refs):
    pos = on_gpu(np.stack([r[0] for r in refs]), torch.int32)
    counts = on_gpu(np.stack([r[1] for r in refs]), torch.int32)
    return pos, counts


def compare_groups(got, refs, what):
    """Positions, counts and distances of the kernel against the restatement's for every reference block whose gap exceeds
    the bound; at most 2 % of the blocks may fall below it."""
    pos, counts, dist = (t.cpu().numpy() for t in got)
    excused = total = 0
    worst = 0.0
    for p, (rpos, rcounts, rdists, gaps, _) in enumerate(refs):
        clear = gaps > 2 * DIST_REL
        excused += int((~clear).sum())
        total += len(gaps)
        for g in np.flatnonzero(clear):
            n = rcounts[g]
            assert counts[p, g] == n, f"{what}: plane {p} block {g}: count {counts[p, g]}, restatement {n}"
            assert np.array_equal(pos[p, g, :n], rpos[g, :n]), f"{what}: plane {p} block {g}: positions differ"
            assert np.all(pos[p, g, n:] == rpos[g, 0]) and np.all(np.isinf(dist[p, g, n:]))
            err = np.abs(dist[p, g, :n] - rdists[g, :n])
            worst = max(worst, float((err / np.maximum(rdists[g, :n], 1e-30)).max()))
            assert np.all(err <= DIST_REL * rdists[g, :n]), f"{what}: plane {p} block {g}: distance error {err.max():.3e}"
    print(f"{what}: {excused} of {total} blocks excused, largest relative distance error {worst:.3e} (bound {DIST_REL:.3e})")
    assert excused <= 0.02 * total, f"{what}: {excused} of {total} reference blocks within the rounding of a decision"


# ---------------------------------------------------------------------------------------------------------------- centring

@pytest.mark.parametrize("shape", [(5, 5), (4, 6)])
@pytest.mark.parametrize("legacy", [False, True])
def test_otf_is_centred_as_the_blur_operators(shape, legacy):
    import physics
    from models.bm3d import otf
    g = torch.Generator().manual_seed(shape[0])
    k = torch.rand(shape, generator=g)
    k = (k / k.sum())[None, None]
    op = physics.Blur(filter=k, padding="circular", device=DEV) if legacy else physics.BlurV2(kernel=k.to(DEV))
    for H, W in ((16, 16), (21, 35)):
        x = torch.rand((1, 2, H, W), generator=g).to(DEV)
        want = torch.fft.fft2(op.A(x))
        got = otf(k.to(DEV), H, W, legacy=legacy) * torch.fft.fft2(x)
        err = float((got - want).abs().max() / want.abs().max())
        print(f"otf {shape} legacy={legacy} at {H} x {W}: relative error {err:.2e}")
        assert err < 1e-5


# ---------------------------------------------------------------------------------------------------------------- matching

# tau: the hard-thresholding default; one so small that some blocks keep only themselves; one that leaves 5 to 7 before the cut
MATCH_CASES = [(H, W, planes, tau, n_max) for (H, W) in EXTENTS for planes in (1, 6)
               for tau, n_max in ((R.TAU_HT, 16), (1.0e-3, 8))] + [(48, 40, 1, R.TAU_WIENER, 32), (21, 35, 1, 6.0e-4, 16)]


@pytest.mark.parametrize("H,W,planes,tau,n_max", MATCH_CASES)
def test_matching_against_the_restatement(H, W, planes, tau, n_max):
    from models.bm3d import bm3d_match
    x, refs = matched(H, W, planes, tau, n_max)
    t = batch_view(x, offset_view=(n_max == 8)) if planes == 6 else on_gpu(x)
    got = bm3d_match(t, tau, n_max, return_distances=True)
    assert got[0].shape == (planes, len(refs[0][1]), n_max, 2) and got[0].dtype == torch.int32
    compare_groups(got, refs, f"match {H} x {W} x {planes} tau {tau:.2e} n_max {n_max}")
    again = bm3d_match(t, tau, n_max, return_distances=True)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "two runs differ"
    if planes == 6:                                                    # a plane alone equals the plane inside the batch
        alone = bm3d_match(on_gpu(x[4]), tau, n_max, return_distances=True)
        assert all(torch.equal(a[0], b[4]) for a, b in zip(alone, got))


def test_matching_cases_cover_the_cuts():
    """The inputs do what the cases are there for (checked on the restatement): counts of 1 at the small tau, and a group of
    5 to 7 cut to 4."""
    singles = cut4 = 0
    for H, W in ((21, 35), (48, 40)):
        for r in matched(H, W, 1, 1.0e-3, 8)[1] + matched(H, W, 6, 1.0e-3, 8)[1]:
            singles += int((r[1] == 1).sum())
            cut4 += int(((r[4] >= 5) & (r[4] <= 7) & (r[1] == 4)).sum())
    print(f"groups of one: {singles}; groups of 5 to 7 cut to 4: {cut4}")
    assert singles > 0 and cut4 > 0


def test_matching_refuses_bad_arguments():
    import _native
    from models.bm3d import bm3d_match
    x = torch.rand((16, 16), device=DEV)
    for kwargs in (dict(n_max=3), dict(n_max=64), dict(step=0), dict(window=38), dict(window=-1), dict(tau=-1.0)):
        args = dict(tau=0.05, n_max=16)
        args.update(kwargs)
        with pytest.raises(ValueError):
            bm3d_match(x, **args)
    with pytest.raises(ValueError):
        bm3d_match(torch.rand((7, 16), device=DEV), 0.05, 16)
    with pytest.raises(_native.NativeLibraryError):
        bm3d_match(torch.rand((16, 16)), 0.05, 16)
    with pytest.raises(_native.NativeLibraryError, match="TOO_LARGE"):
        bm3d_match(x, 0.05, 16, window=91)


# --------------------------------------------------------------------------------------------------------------- filtering

def variances_of(planes, seed):
    """Coefficient variances of a coloured spectrum around (0.02)^2, float32 values as float64 (planes, 64)."""
    rng = np.random.default_rng(seed)
    v = 0.02 ** 2 * (0.5 + 1.5 * rng.random((planes, 64)))
    return v.astype(np.float32).astype(np.float64)


def touched(H, W, pos, counts, groups):
    mask = np.zeros((H, W), dtype=bool)
    for g in groups:
        for r, c in pos[g, :counts[g]]:
            mask[r:r + 8, c:c + 8] = True
    return mask


FILTER_CASES = [(H, W, 1, n_max) for (H, W) in EXTENTS for n_max in (16, 32)] + [(48, 40, 6, 16), (21, 35, 6, 32)]


@pytest.mark.parametrize("agg", [0, 1])
@pytest.mark.parametrize("H,W,planes,n_max", FILTER_CASES)
def test_hard_thresholding_on_injected_groups(H, W, planes, n_max, agg):
    from models.bm3d import bm3d_ht
    tau = R.TAU_HT if n_max == 16 else 2 * R.TAU_HT
    x, refs = matched(H, W, planes, tau, n_max)
    var = variances_of(planes, H)
    t = batch_view(x, offset_view=True) if planes == 6 else on_gpu(x)
    out, coef = bm3d_ht(t, on_gpu(var), groups=groups_on_gpu(refs), agg=agg, return_coefficients=True)
    out, coef = out.reshape(planes, H, W).cpu().numpy().astype(np.float64), coef.cpu().numpy().astype(np.float64)
    worst_coef = worst_out = 0.0
    excused = 0
    for p in range(planes):
        pos, counts = refs[p][0], refs[p][1]
        want, margins, rcoef = R.ht_ref(x[p], var[p], pos, counts)
        thr = R.LAMBDA_3D * np.sqrt(var[p])
        for g, n in enumerate(counts):
            near = np.abs(rcoef[g, :n]) < 2 * thr
            err = np.abs(coef[p, g, :n] - rcoef[g, :n]) / thr
            worst_coef = max(worst_coef, float(err[near].max()) if near.any() else 0.0)
        mask = touched(H, W, pos, counts, np.flatnonzero(margins < COEF_ERR))
        excused += int(mask.sum())
        diff = np.abs(out[p] - want)
        worst_out = max(worst_out, float(diff[~mask].max()) if (~mask).any() else 0.0)
    print(f"ht {H} x {W} x {planes} n_max {n_max} agg {agg}: coefficient error / threshold {worst_coef:.3e} (COEF_ERR "
          f"{COEF_ERR:.1e}), output error {worst_out:.3e} (OUT_TOL {OUT_TOL:.1e}), {excused} of {planes * H * W} pixels excused")
    assert worst_coef <= COEF_ERR
    assert excused <= 0.05 * planes * H * W
    assert worst_out <= OUT_TOL


@pytest.mark.parametrize("agg", [0, 1])
@pytest.mark.parametrize("H,W,planes,n_max", FILTER_CASES)
def test_wiener_on_injected_groups(H, W, planes, n_max, agg):
    from models.bm3d import bm3d_wiener
    tau = R.TAU_HT if n_max == 16 else 2 * R.TAU_HT
    x, refs = matched(H, W, planes, tau, n_max)
    var = variances_of(planes, H + 1)
    pilot = np.clip(R.smooth_image(H, W, 0, planes) + 0.005 * np.random.default_rng(H).standard_normal((planes, H, W)), 0, 1)
    pilot = pilot.astype(np.float32).astype(np.float64)
    t = batch_view(x, offset_view=True) if planes == 6 else on_gpu(x)
    out = bm3d_wiener(t, on_gpu(pilot).reshape(t.shape), on_gpu(var), groups=groups_on_gpu(refs), agg=agg)
    out = out.reshape(planes, H, W).cpu().numpy().astype(np.float64)
    worst = max(float(np.abs(out[p] - R.wiener_ref(x[p], pilot[p], var[p], refs[p][0], refs[p][1])).max())
                for p in range(planes))
    print(f"wiener {H} x {W} x {planes} n_max {n_max} agg {agg}: output error {worst:.3e} (OUT_TOL {OUT_TOL:.1e})")
    assert worst <= OUT_TOL


@pytest.mark.parametrize("agg", [0, 1])
@pytest.mark.parametrize("H,W", EXTENTS)
def test_zero_threshold_returns_the_input(H, W, agg):
    """Coverage and aggregation: with lambd = 0 every coefficient is kept and num / den is a weighted mean of copies of the
    input, with the kernel's own matching."""
    from models.bm3d import bm3d_ht
    x = on_gpu(planes_of(H, W, 3, seed=7))
    out = bm3d_ht(x, on_gpu(variances_of(3, 1)), lambd=0.0, agg=agg)
    err = float((out - x).abs().max())
    print(f"lambd = 0 at {H} x {W} agg {agg}: largest change {err:.3e}")
    assert out.shape == x.shape and err <= OUT_TOL


def test_injected_groups_are_validated_on_the_host():
    """Out-of-range positions, counts that are no power of two in [1, n_max], wrong dtypes, shapes and devices raise in the
    Python layer (every message names the caller): nothing is launched."""
    import _native
    from models.bm3d import bm3d_ht, bm3d_wiener
    H, W = 21, 35
    x, refs = matched(H, W, 1, R.TAU_HT, 16)
    t, var = on_gpu(x), on_gpu(variances_of(1, 0))
    pos, counts = groups_on_gpu(refs)
    bm3d_ht(t, var, groups=(pos, counts))
    bad = []
    for at, value in (((0, 3, 1, 0), H - 7), ((0, 3, 1, 0), -1), ((0, 59, 0, 1), W - 7), ((0, 0, 15, 1), 1 << 30)):
        p = pos.clone()
        p[at] = value
        bad.append((p, counts))
    for value in (0, 3, 17, 32, -4):
        c = counts.clone()
        c[0, 5] = value
        bad.append((pos, c))
    bad += [(pos.long(), counts), (pos, counts.float()), (pos[:, :-1], counts[:, :-1]), (pos[..., :1], counts),
            (pos.cpu(), counts.cpu()), (pos[:, :, :12], counts)]
    for groups in bad:
        with pytest.raises((ValueError, TypeError, _native.NativeLibraryError), match="bm3d_ht"):
            bm3d_ht(t, var, groups=groups)
        with pytest.raises((ValueError, TypeError, _native.NativeLibraryError), match="bm3d_wiener"):
            bm3d_wiener(t, t, var, groups=groups)
    with pytest.raises(ValueError, match="positions outside"):
        bm3d_ht(t, var, groups=bad[0])


# ------------------------------------------------------------------------------------------------------------------- chain

_CHAIN = {}


def e2e_case(seed, planes=3, H=48, W=40):
    """(x, y, kernel): a ground truth with steep edges, its Gaussian_R2 blur plus noise at 5 / 255 as float32 values, the
    kernel. (The seeds are ones at which the restatement itself improves on the measurement: with variances per 2-D
    coefficient its Wiener stage under-shrinks the correlated noise of neighbouring blocks, and at this extent that does not
    hold for every image.)"""
    from oracle.torch_path import blur_fft, blur_kernel
    x = R.edged_image(H, W, seed, planes)
    k = blur_kernel("Gaussian_R2")
    y = blur_fft(torch.from_numpy(x), k).numpy() + SIGMA * np.random.default_rng(200 + seed).standard_normal(x.shape)
    return x, y.astype(np.float32).astype(np.float64), k.numpy()


def chain(seed):
    if seed not in _CHAIN:
        x, y, k = e2e_case(seed)
        _CHAIN[seed] = (x, y, k, [R.deblur_ref(y[p], k, SIGMA) for p in range(y.shape[0])])
    return _CHAIN[seed]


def test_chain_of_the_four_steps():
    """Each GPU stage is fed the restatement's previous-stage output cast to float32 and compared with the restatement's next
    one: decisions cannot compound."""
    from models.bm3d import bm3d_ht, bm3d_match, bm3d_wiener, otf, regularised_inverse
    x, y, k, ts = chain(E2E_SEEDS[0])
    planes, H, W = y.shape
    stack = lambda key: np.stack([t[key] for t in ts])                                      # noqa: E731
    f32 = lambda a: a.astype(np.float32).astype(np.float64)                                 # noqa: E731
    V = otf(on_gpu(k, torch.float64), H, W, dtype=torch.float64)
    # step 1
    z1, v1 = regularised_inverse(on_gpu(y), V, SIGMA)
    e_z, e_v = float(np.abs(z1.cpu().numpy() - stack("z1")).max() / np.abs(stack("z1")).max()), \
        float((np.abs(v1.cpu().numpy() - stack("v1")) / stack("v1").max()).max())
    print(f"step 1: z1 relative error {e_z:.2e}, variances {e_v:.2e} (INVERSE_TOL {INVERSE_TOL:.1e})")
    assert e_z <= INVERSE_TOL and e_v <= INVERSE_TOL
    # step 2 on the restatement's z1: matching, then the filter on the restatement's groups
    z1r, v1r = f32(stack("z1")), f32(stack("v1"))
    refs1 = [R.match_ref(z1r[p], R.TAU_HT, R.N_MAX_HT) for p in range(planes)]
    compare_groups(bm3d_match(on_gpu(z1r), R.TAU_HT, R.N_MAX_HT, return_distances=True), refs1, "chain step 2")
    pilot = bm3d_ht(on_gpu(z1r), on_gpu(v1r), groups=groups_on_gpu(refs1)).cpu().numpy()
    excused, worst = 0, 0.0
    for p in range(planes):
        want, margins, _ = R.ht_ref(z1r[p], v1r[p], refs1[p][0], refs1[p][1])
        mask = touched(H, W, refs1[p][0], refs1[p][1], np.flatnonzero(margins < COEF_ERR))
        excused += int(mask.sum())
        worst = max(worst, float(np.abs(pilot[p] - want)[~mask].max()))
    print(f"step 2: pilot error {worst:.3e} (OUT_TOL {OUT_TOL:.1e}), {excused} of {planes * H * W} pixels excused")
    assert excused <= 0.05 * planes * H * W and worst <= OUT_TOL
    # step 3 on the restatement's pilot
    pr = f32(stack("pilot"))
    z2, v2 = regularised_inverse(on_gpu(y), V, SIGMA, pilot=on_gpu(pr))
    want = [R.inverse_ref(y[p], R.otf_ref(k, H, W), SIGMA ** 2, pr[p]) for p in range(planes)]
    want_z2 = np.stack([w[0] for w in want])
    want_v2 = np.stack([R.coefficient_variances_ref(w[1]) for w in want])
    e_z = float(np.abs(z2.cpu().numpy() - want_z2).max() / np.abs(want_z2).max())
    e_v = float((np.abs(v2.cpu().numpy() - want_v2) / want_v2.max()).max())
    print(f"step 3: z2 relative error {e_z:.2e}, variances {e_v:.2e} (INVERSE_TOL {INVERSE_TOL:.1e})")
    assert e_z <= INVERSE_TOL and e_v <= INVERSE_TOL
    # step 4 on the restatement's z2, pilot and variances
    z2r, v2r = f32(stack("z2")), f32(stack("v2"))
    refs2 = [R.match_ref(pr[p], R.TAU_WIENER, R.N_MAX_WIENER) for p in range(planes)]
    compare_groups(bm3d_match(on_gpu(pr), R.TAU_WIENER, R.N_MAX_WIENER, return_distances=True), refs2, "chain step 4")
    out = bm3d_wiener(on_gpu(z2r), on_gpu(pr), on_gpu(v2r), groups=groups_on_gpu(refs2)).cpu().numpy()
    worst = max(float(np.abs(out[p] - R.wiener_ref(z2r[p], pr[p], v2r[p], refs2[p][0], refs2[p][1])).max())
                for p in range(planes))
    print(f"step 4: output error {worst:.3e} (OUT_TOL {OUT_TOL:.1e})")
    assert worst <= OUT_TOL


# -------------------------------------------------------------------------------------------------------------- end to end

@pytest.mark.parametrize("seed", E2E_SEEDS)
def test_forward_against_the_restatement(seed):
    """BM3D.forward on a (1, 3, 48, 40) measurement against the float64 restatement by RMS difference. The restatement in
    float32 against itself in float64 differs by RMS 8.859e-06, 2.516e-05 and 2.716e-07 at the seeds 1, 2, 3 (a
    decision or two flip at the first two); E2E_RMS is twice the largest."""
    import physics
    from models.bm3d import BM3D
    x, y, k, ts = chain(seed)
    model = BM3D(physics.BlurV2(kernel=on_gpu(k)[None, None]), SIGMA)
    out = model(on_gpu(y)[None])
    assert out.shape == (1,) + y.shape and len(model.state_dict()) == 0
    out = out[0].cpu().numpy().astype(np.float64)
    want = np.stack([t["out"] for t in ts])
    rms = lambda a, b: float(np.sqrt(((a - b) ** 2).mean()))                                # noqa: E731
    print(f"seed {seed}: RMS to the restatement {rms(out, want):.3e} (E2E_RMS {E2E_RMS:.1e}); to the ground truth: "
          f"measurement {rms(y, x):.4f}, output {rms(out, x):.4f}")
    assert rms(out, x) < rms(y, x)
    assert rms(out, want) <= E2E_RMS


def run_test_py(*flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), "--device", "cuda", "--dataset", "synthetic",
                           "--indices", "0", "--model_kind", "BM3D", *flags], capture_output=True, text=True, timeout=300)


def test_test_py_runs_the_bm3d_baseline():
    r = run_test_py("--task", "deblurring", "--kernel", "Gaussian_R2")
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert "N: 1" in lines
    assert math.isfinite(float([ln for ln in lines if ln.startswith("PSNR:")][0].split()[-1]))


def test_test_py_refuses_super_resolution():
    r = run_test_py("--task", "sr", "--sr_factor", "2")
    assert r.returncode != 0 and "NotImplementedError" in r.stderr and "outside" in r.stderr
