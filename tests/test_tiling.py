"""CPU: the tiling plan and windows of tiling.py against brute force, tests/tiling_ref.py against images it must reproduce,
and test.py's --tile flags (parse_args refuses before any GPU object exists)."""
import os
import sys

import pytest
import torch

import tiling
import tiling_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_origins(n, T, v):
    """The definition, step by step."""
    if n <= T:
        return [0]
    out, o = [], 0
    while o < n - T:
        out.append(o)
        o += T - v
    return out + [n - T]


def brute_weight(kind, n, Te, v, o, i):
    if kind == "uniform":
        return 1
    if kind == "feather":
        return min(i + 1, Te - i, max(v, 1))
    lo = 0 if o == 0 else v // 2
    hi = 0 if o + Te == n else v - v // 2
    return 1 if lo <= i < Te - hi else 0


def sweep(t_max, n_max):
    for T in range(1, t_max):
        for v in range(0, T // 2 + 1):
            for n in range(1, n_max):
                yield n, T, v


def test_plan_and_windows_against_brute_force():
    for n, T, v in sweep(20, 70):
        origins, Te, stride = tiling.tile_plan(n, T, v)
        assert origins == brute_origins(n, T, v) == R.plan(n, T, v)[0], (n, T, v)
        assert Te == min(n, T) == R.plan(n, T, v)[1] and 1 <= stride <= Te
        assert all(b > a for a, b in zip(origins, origins[1:])), (n, T, v)           # strictly increasing
        assert origins[0] == 0 and origins[-1] + Te == n, (n, T, v)                   # the last tile ends on the border
        if len(origins) > 1:
            assert stride == T - v and origins[:-1] == [k * stride for k in range(len(origins) - 1)]
            assert (len(origins) - 2) * stride < n - T <= (len(origins) - 1) * stride  # what the kernels re-derive
        cover = [0] * n
        for o in origins:
            for i in range(Te):
                cover[o + i] += 1
        assert min(cover) >= 1 and max(cover) <= 3, (n, T, v)                         # 2 v <= T: at most three tiles
        for kind in tiling.WINDOWS:
            total = [0] * n
            for o in origins:
                w = tiling.axis_weights(kind, n, Te, stride, o)
                assert w == [brute_weight(kind, n, Te, v, o, i) for i in range(Te)], (kind, n, T, v, o)
                assert w == R.weights(kind, n, Te, v, o).long().tolist()
                for i in range(Te):
                    total[o + i] += w[i]
            assert min(total) >= 1, (kind, n, T, v)                                   # positive weight everywhere


def test_three_tiles_at_the_most_on_a_wider_sweep():
    for n, T, v in sweep(40, 200):
        origins, Te, _ = tiling.tile_plan(n, T, v)
        edges = [0] * (n + 1)
        for o in origins:
            edges[o] += 1
            edges[o + Te] -= 1
        depth = worst = 0
        for e in edges:
            depth += e
            worst = max(worst, depth)
        assert 1 <= worst <= 3, (n, T, v)


def test_crop_cores_of_the_regular_tiles_partition_the_axis():
    """Every tile but the shifted last one: the cores are disjoint, and together with the last tile's they leave no hole;
    where the last tile sits on the regular grid as well (n - T a multiple of the stride) all cores partition the axis."""
    for n, T, v in sweep(20, 70):
        origins, Te, stride = tiling.tile_plan(n, T, v)
        regular = origins[:-1] if len(origins) > 1 else origins
        count = [0] * n
        for o in regular:
            for i, w in enumerate(tiling.axis_weights("crop", n, Te, stride, o)):
                count[o + i] += w
        assert max(count) <= 1, (n, T, v)                                             # disjoint
        covered = [c for c in count]
        if len(origins) > 1:
            # the regular cores are one interval from 0 up to the upper margin of the last regular tile
            end = regular[-1] + Te - (v - v // 2)
            assert count == [1] * end + [0] * (n - end), (n, T, v)
            for i, w in enumerate(tiling.axis_weights("crop", n, Te, stride, origins[-1])):
                covered[origins[-1] + i] += w
            assert min(covered) >= 1
            if (n - T) % stride == 0:
                assert covered == [1] * n, (n, T, v)
        else:
            assert count == [1] * n


def test_plan_refuses_bad_arguments():
    for bad in ((0, 8, 0), (8, 0, 0), (8, 8, -1), (8, 8, 5)):
        with pytest.raises(ValueError):
            tiling.tile_plan(*bad)
    with pytest.raises(ValueError):
        tiling.axis_weights("hann", 8, 8, 8, 0)
    for kwargs in (dict(tile=0), dict(tile=4096), dict(tile=16, overlap=9), dict(tile=16, batch=0),
                   dict(tile=16, scale=0), dict(tile=1024, scale=4), dict(tile=16, window="hann")):
        with pytest.raises(ValueError):
            tiling.TiledModel(lambda v: v, **kwargs)


SHAPES = [(1, 8, 8, 8, 0), (3, 5, 9, 8, 2), (3, 9, 9, 8, 4), (3, 16, 24, 8, 0), (3, 19, 23, 8, 3), (1, 33, 70, 16, 8),
          (3, 48, 40, 16, 6)]


@pytest.mark.parametrize("C,H,W,T,v", SHAPES)
def test_reference_reproduces_constant_and_affine_images(C, H, W, T, v):
    """A partition of unity: through the identity model every window returns the image. 1e-12 in float64."""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    ramp = torch.stack([0.25 + 0.5 * c + 0.03 * yy - 0.07 * xx for c in range(C)])
    const = torch.full((C, H, W), 0.4, dtype=torch.float64)
    for kind in R.WINDOWS:
        for image in (const, ramp):
            got = R.tiled(lambda t: t, image, T, v, kind)
            assert got.shape == image.shape and float((got - image).abs().max()) <= 1e-12, (kind, C, H, W, T, v)
    # and the blend of scaled tiles lands on the scaled image
    for scale in (2, 4):
        up = lambda t: t.repeat_interleave(scale, -1).repeat_interleave(scale, -2)
        got = R.tiled(up, ramp, T, v, "feather", scale=scale)
        assert float((got - up(ramp)).abs().max()) <= 1e-12


def test_reference_gather_is_slicing_in_tile_order():
    x = torch.arange(3 * 19 * 23, dtype=torch.float64).view(3, 19, 23)
    tiles = R.gather(x, 8, 3)
    origins, Th, Tw = R.tiles_of(19, 23, 8, 3)
    assert (Th, Tw) == (8, 8) and origins[:5] == [(0, 0), (0, 5), (0, 10), (0, 15), (5, 0)] and origins[-1] == (11, 15)
    assert tiles.shape == (16, 3, 8, 8) and torch.equal(tiles[5], x[:, 5:13, 5:13])


# ------------------------------------------------------------------------------------------------ test.py's flags
@pytest.fixture(scope="module")
def driver():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sei_test_driver", os.path.join(ROOT, "test.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


BASE = ["--device", "cuda", "--task", "deblurring", "--kernel", "Gaussian_R2"]


def test_command_line_without_tile_parses_to_off(driver):
    args = driver.parse_args(BASE)
    assert args.tile == 0 and args.tile_overlap == 32 and args.tile_batch == 8 and args.tile_window == "feather"


def test_tile_flags_parse(driver):
    args = driver.parse_args(BASE + ["--tile", "256", "--tile_overlap", "16", "--tile_batch", "4", "--tile_window", "crop"])
    assert (args.tile, args.tile_overlap, args.tile_batch, args.tile_window) == (256, 16, 4, "crop")
    assert driver.tile_scale(args) == 1
    sr = ["--device", "cuda", "--task", "sr", "--sr_factor", "2", "--tile", "64"]
    assert driver.tile_scale(driver.parse_args(sr)) == 2
    assert driver.tile_scale(driver.parse_args(sr + ["--model_kind", "Upsample"])) == 2
    assert driver.tile_scale(driver.parse_args(sr + ["--model_kind", "Identity"])) == 1
    assert driver.parse_args(BASE + ["--tile", "64", "--tile_overlap", "32"]).tile_overlap == 32      # 2 V == T is allowed


@pytest.mark.parametrize("flags,named", [
    (["--tile", "40"], "--tile"),                                    # not a multiple of 16
    (["--tile", "-16"], "--tile"),
    (["--tile", "2064"], "--tile"),                                  # above 2048
    (["--tile", "48", "--tile_overlap", "25"], "--tile_overlap"),    # 2 V > T
    (["--tile", "16"], "--tile_overlap"),                            # the default overlap of 32 does not fit
    (["--tile", "64", "--tile_overlap", "-1"], "--tile_overlap"),
    (["--tile", "64", "--tile_batch", "0"], "--tile_batch"),
    (["--tile", "64", "--tile_window", "hann"], "--tile_window"),
    (["--tile", "64", "--model_kind", "TV"], "--tile"),
    (["--tile", "64", "--model_kind", "InverseFilter"], "--tile"),
    (["--tile", "64", "--model_kind", "DeepImagePrior"], "--tile"),
    (["--tile", "64", "--model_kind", "PlugAndPlay"], "--tile"),
    (["--tile", "64", "--model_kind", "DiffPIR_DRUNet"], "--tile"),
    (["--tile", "64", "--model_kind", "DiffPIR_DiffUNet"], "--tile"),
    (["--tile", "64", "--model_kind", "DPS"], "--tile"),
    (["--tile", "64", "--model_kind", "BM3D"], "--tile"),
])
def test_parse_args_refuses_by_the_flags_name(driver, capsys, flags, named):
    with pytest.raises(SystemExit) as stop:
        driver.parse_args(BASE + flags)
    assert stop.value.code == 2
    message = capsys.readouterr().err.splitlines()[-1]
    assert f"argument {named}" in message or f"error: {named} " in message, message


def test_parse_args_refuses_a_tile_beyond_the_kernels_extent_after_upsampling(driver, capsys):
    with pytest.raises(SystemExit):
        driver.parse_args(["--device", "cuda", "--task", "sr", "--sr_factor", "4", "--tile", "1024"])
    assert "--tile" in capsys.readouterr().err


def test_entry_points_refuse_bad_plans_on_the_host():
    """Host arithmetic before any HIP call: fake pointers are never dereferenced because nothing is launched."""
    import _native
    L = _native.lib()
    P, Q = 4096, 1 << 20
    ok = dict(x=P, tiles=Q, C=3, H=19, W=23, Th=8, Tw=8, sy=5, sx=5, ny=4, nx=4, t0=0, n=16, stream=None)
    for change in (dict(x=None), dict(tiles=None), dict(x=P + 2), dict(C=0), dict(H=0), dict(Th=0), dict(sy=0), dict(ny=0),
                   dict(ny=3), dict(ny=5), dict(nx=3), dict(sy=3, ny=5), dict(sx=9), dict(H=8, ny=2), dict(H=6, ny=1),
                   dict(t0=-1), dict(n=0), dict(n=17), dict(t0=1), dict(tiles=P + 64), dict(x=Q + 64),
                   dict(H=4096, W=4096, Th=4096, Tw=4096, sy=4096, sx=4096, ny=1, nx=1, n=1),
                   dict(H=1 << 15, W=1 << 15, Th=2048, Tw=2048, sy=2048, sx=2048, ny=16, nx=16, n=1, tiles=1 << 40)):
        args = dict(ok, **change)
        assert L.sei_tile_gather(*args.values()) == 10001, change
        blend = dict(tiles=args["tiles"], out=args["x"], **{k: args[k] for k in ("C", "H", "W", "Th", "Tw", "sy", "sx", "ny",
                                                                                 "nx")},
                     window=1, t0=args["t0"], n=args["n"], accumulate=0, finish=1, stream=None)
        assert L.sei_tile_blend(*blend.values()) == 10001, change
    for window in (-1, 3):
        assert L.sei_tile_blend(Q, P, 3, 19, 23, 8, 8, 5, 5, 4, 4, window, 0, 16, 0, 1, None) == 10001
