"""GPU: the tiling kernels (sei_tile_gather, sei_tile_blend), the host class around them (tiling.TiledModel) and
test.py --tile, against tests/tiling_ref.py.

Bars: tests/streaming_ref.py's (`same_bits`; `hold32`: within max(5e-6, 3 * ref32) of float64, ref32 the deviation of the same
torch chain in float32). Outputs are `Guarded`, inputs NaN-tailed, as in tests/test_bootstrap_gpu.py.

Shapes (C, H, W, T, v), the smallest at which each rule of the plan can go wrong: one tile; an axis shorter than the tile;
a last tile shifted by one pixel; an exact multiple without overlap; an odd overlap (crop's two margins differ); 2 v == T
(three tiles cover a pixel); and one that is also blended scaled by 2 and by 4.

Measured on an MI355X (the largest over the cases of each row; deviation and ref32 relative to max |ref64|; the bar is the
floor of 5e-6 in every row):

  quantity                                                  ref32     HIP deviation
  blend uniform / feather / crop, the seven shapes, x2, x4  1.0e-7 / 1.4e-7 / 7.2e-8    1.0e-7 / 1.4e-7 / 7.2e-8
  TiledModel around the identity, all windows               9.6e-8    9.6e-8 (0 under crop and without overlap)
  TiledModel crop around the 5 x 5 box filter               2.1e-7    5.9e-8
  TiledModel(scale=2) around Upsample, away from the seams  1.0e-7    1.0e-7
  peak memory, small U-Net on 256 x 256, T = 64, batch 1    tiled 2.9 MB above the 412 MB resident before the call, whole
                                                            33.6 MB above it (0.931 of the whole-image peak in total)
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _native as N
import streaming_ref as S
import tiling
import tiling_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = 10001

SHAPES = [(1, 8, 8, 8, 0), (3, 5, 9, 8, 2), (3, 9, 9, 8, 4), (3, 16, 24, 8, 0), (3, 19, 23, 8, 3), (1, 33, 70, 16, 8),
          (3, 48, 40, 16, 6)]
SCALED = [(*SHAPES[-1], 2), (*SHAPES[-1], 4)]
WINDOWS = R.WINDOWS


def plan_args(H, W, T, v, scale=1):
    """(H, W, Th, Tw, sy, sx, ny, nx) as the entry points take them, for the image and the plan times `scale`."""
    (oy, Th, sy), (ox, Tw, sx) = tiling.tile_plan(scale * H, scale * T, scale * v), tiling.tile_plan(scale * W, scale * T,
                                                                                                    scale * v)
    return scale * H, scale * W, Th, Tw, sy, sx, len(oy), len(ox)


def chunks(total, chunk):
    """(t0, n) of consecutive chunks of `chunk` tiles (0: all at once)."""
    step = chunk or total
    return [(t0, min(step, total - t0)) for t0 in range(0, total, step)]


def image(C, H, W, seed=0):
    return torch.rand((C, H, W), generator=torch.Generator().manual_seed(seed + 100 * H + W)) * 1.5 - 0.25


def off_grid(shape, lead):
    """A Guarded output whose view starts `lead` floats past the 16-byte grid -> (guard, view)."""
    g = S.Guarded((math.prod(shape) + lead,))
    return g, g.view[lead:].view(shape)


def gather(x, T, v, chunk=0, lead=0):
    C, H, W = x.shape
    plan = plan_args(H, W, T, v)
    total = plan[-1] * plan[-2]
    guard, tiles = off_grid((total, C, plan[2], plan[3]), lead)
    xd = S.nan_tailed(x)
    for t0, n in chunks(total, chunk):
        N.call("sei_tile_gather", xd.data_ptr(), tiles[t0:].data_ptr(), C, *plan, t0, n)
    torch.cuda.synchronize()
    assert guard.intact() and bool((guard.view[:lead] == S.SENTINEL).all())
    return tiles.cpu()


def blend(tiles, H, W, T, v, kind, scale=1, chunk=0, lead=0, in_lead=0):
    """sei_tile_blend over CPU tiles (total, C, scale Th, scale Tw) -> (C, scale H, scale W) on the CPU."""
    total, C = tiles.shape[:2]
    plan = plan_args(H, W, T, v, scale)
    assert total == plan[-1] * plan[-2] and tuple(tiles.shape[2:]) == plan[2:4]
    guard, out = off_grid((C, plan[0], plan[1]), lead)
    td = S.nan_framed(tiles, in_lead)
    for t0, n in chunks(total, chunk):
        N.call("sei_tile_blend", td[t0:].data_ptr(), out.data_ptr(), C, *plan, WINDOWS.index(kind), t0, n, int(t0 > 0),
               int(t0 + n == total))
    torch.cuda.synchronize()
    assert guard.intact() and bool((guard.view[:lead] == S.SENTINEL).all())
    return out.cpu()


def random_tiles(C, H, W, T, v, scale=1):
    plan = plan_args(H, W, T, v, scale)
    gen = torch.Generator().manual_seed(7 * H + W + scale)
    return torch.rand((plan[-1] * plan[-2], C, plan[2], plan[3]), generator=gen) * 1.5 - 0.25


# ------------------------------------------------------------------------------------------------ sei_tile_gather
@pytest.mark.parametrize("C,H,W,T,v", SHAPES)
def test_gather_is_slicing_bit_for_bit(C, H, W, T, v):
    x = image(C, H, W)
    want = R.gather(x, T, v)
    for chunk, lead in ((0, 0), (1, 1), (3, 0), (3, 3)):
        assert S.same_bits(gather(x, T, v, chunk, lead), want), (chunk, lead)


# ------------------------------------------------------------------------------------------------ sei_tile_blend
@pytest.mark.parametrize("kind", WINDOWS)
@pytest.mark.parametrize("C,H,W,T,v,scale", [(*s, 1) for s in SHAPES] + SCALED)
def test_blend_against_float64(C, H, W, T, v, scale, kind):
    tiles = random_tiles(C, H, W, T, v, scale)
    got = blend(tiles, H, W, T, v, kind, scale)
    S.hold32(f"blend {kind} {C}x{H}x{W} T={T} v={v} x{scale}", got, R.blend(tiles, H, W, T, v, kind, scale),
             R.blend(tiles, H, W, T, v, kind, scale, dtype=torch.float32))


# without overlap every window weighs every pixel once, by 1; under crop the regular cores do that whatever the overlap
ONE_TILE_CASES = [(*s, kind) for s in SHAPES if s[-1] == 0 for kind in WINDOWS if kind != "crop"] + \
    [(*s, "crop") for s in SHAPES]


@pytest.mark.parametrize("C,H,W,T,v,kind", ONE_TILE_CASES)
def test_blend_where_one_tile_counts_is_that_tile(C, H, W, T, v, kind):
    """Weight 1 over weight sum 1: fmaf(1, value, 0) / 1 is the value. Every pixel of the shapes without overlap under any
    window; under crop the pixels outside the shifted last tiles of every shape (the regular cores partition them)."""
    count, in_last = R.coverage(H, W, T, v, kind)
    once = (count == 1) & ~in_last
    assert bool((count[~in_last] == 1).all())
    if v == 0 and H % T == 0 and W % T == 0:
        once = count == 1
        assert bool(once.all())
    tiles = random_tiles(C, H, W, T, v)
    got = blend(tiles, H, W, T, v, kind)
    origins, Th, Tw = R.tiles_of(H, W, T, v)
    want = torch.full((C, H, W), float("nan"))
    for tile, (a, b) in zip(tiles, origins):                  # the tile that owns the pixel, by its non-zero weight
        w = R.weights(kind, H, Th, v, a)[:, None] * R.weights(kind, W, Tw, v, b)[None, :]
        region = want[:, a:a + Th, b:b + Tw]
        region[:, w != 0] = tile[:, w != 0]
    assert bool(once.any())
    assert S.same_bits(got[:, once], want[:, once])


@pytest.mark.parametrize("kind", WINDOWS)
@pytest.mark.parametrize("C,H,W,T,v,scale", [(*s, 1) for s in SHAPES] + SCALED[:1])
def test_blend_chunked_and_off_grid_calls_leave_the_bits_of_one_call(C, H, W, T, v, scale, kind):
    tiles = random_tiles(C, H, W, T, v, scale)
    whole = blend(tiles, H, W, T, v, kind, scale)
    assert S.same_bits(blend(tiles, H, W, T, v, kind, scale, chunk=1), whole)
    assert S.same_bits(blend(tiles, H, W, T, v, kind, scale, chunk=3), whole)
    assert S.same_bits(blend(tiles, H, W, T, v, kind, scale, lead=1), whole)              # out 4 bytes off the grid
    assert S.same_bits(blend(tiles, H, W, T, v, kind, scale, chunk=3, lead=3, in_lead=1), whole)


def test_refusals_leave_out_untouched():
    C, H, W, T, v = 3, 19, 23, 8, 3
    plan = plan_args(H, W, T, v)
    assert plan == (19, 23, 8, 8, 5, 5, 4, 4)
    tiles = S.nan_tailed(random_tiles(C, H, W, T, v))
    out, x = S.Guarded((C, H, W)), S.nan_tailed(image(C, H, W))
    tiles_out = S.Guarded((16, C, 8, 8))
    names = ("C", "H", "W", "Th", "Tw", "sy", "sx", "ny", "nx")
    ok = dict(zip(names, (C, *plan)), window=1, t0=0, n=16)
    L, stream = N.lib(), N.stream()
    bad = [dict(C=0), dict(H=0), dict(W=-1), dict(Th=0), dict(sy=0), dict(ny=0), dict(nx=0), dict(ny=3), dict(ny=5),
           dict(nx=5), dict(sy=3), dict(sx=9), dict(Th=2064, H=2064, ny=1, sy=2064),
           dict(H=8, ny=2), dict(H=6, ny=1), dict(t0=-1), dict(n=0), dict(n=17), dict(t0=1), dict(window=3),
           dict(window=-1)]
    for change in bad:
        a = dict(ok, **change)
        geometry = [a[k] for k in names]
        rc = L.sei_tile_blend(tiles.data_ptr(), out.ptr(), *geometry, a["window"], a["t0"], a["n"], 0, 1, stream)
        assert rc == BAD_ARG, change
        if "window" not in change:
            rc = L.sei_tile_gather(x.data_ptr(), tiles_out.ptr(), *geometry, a["t0"], a["n"], stream)
            assert rc == BAD_ARG, change
    geometry = [ok[k] for k in names]
    assert L.sei_tile_blend(None, out.ptr(), *geometry, 1, 0, 16, 0, 1, stream) == BAD_ARG
    assert L.sei_tile_blend(tiles.data_ptr(), None, *geometry, 1, 0, 16, 0, 1, stream) == BAD_ARG
    assert L.sei_tile_blend(out.ptr() + 64, out.ptr(), *geometry, 1, 0, 16, 0, 1, stream) == BAD_ARG    # tiles overlap out
    assert L.sei_tile_gather(None, tiles_out.ptr(), *geometry, 0, 16, stream) == BAD_ARG
    assert L.sei_tile_gather(tiles_out.ptr() + 128, tiles_out.ptr(), *geometry, 0, 16, stream) == BAD_ARG
    # 2^30 pixels per plane: a valid plan of a 32768 x 32768 image (nothing is launched, so nothing that large is touched)
    huge = (3, 1 << 15, 1 << 15, 2048, 2048, 2048, 2048, 16, 16)
    assert L.sei_tile_blend(tiles.data_ptr(), out.ptr(), *huge, 1, 0, 1, 0, 1, stream) == BAD_ARG
    torch.cuda.synchronize()
    for g in (out, tiles_out):
        assert g.intact() and bool((g.view == S.SENTINEL).all())


# ------------------------------------------------------------------------------------------------ the host class
@pytest.mark.parametrize("kind", WINDOWS)
@pytest.mark.parametrize("C,H,W,T,v", SHAPES)
def test_tiled_identity_returns_the_image(C, H, W, T, v, kind):
    y = image(C, H, W, seed=3)
    ref32 = R.tiled(lambda t: t, y, T, v, kind, dtype=torch.float32)
    outs = []
    for batch in (1, 5):
        got = tiling.TiledModel(lambda t: t, tile=T, overlap=v, batch=batch, window=kind)(y.cuda())
        assert got.shape == y.shape
        S.hold32(f"TiledModel identity {kind} {C}x{H}x{W} batch {batch}", got, y.double(), ref32)
        outs.append(got)
    assert S.same_bits(outs[0], outs[1])
    if v == 0 and (H, W) == (16, 24):
        assert S.same_bits(outs[0], y)
    batched = tiling.TiledModel(lambda t: t, tile=T, overlap=v, batch=5, window=kind)(torch.stack([y, y.flip(-1)]).cuda())
    assert batched.shape == (2, C, H, W) and S.same_bits(batched[0], outs[0])
    S.hold32("the second image of a batch", batched[1], y.flip(-1).double(), ref32.flip(-1))


def test_tiled_model_refuses_cpu_tensors():
    with pytest.raises(N.NativeLibraryError):
        tiling.TiledModel(lambda t: t, tile=8, overlap=0)(torch.rand(3, 16, 16))


def box_filter(channels, dtype, device):
    return torch.full((channels, 1, 5, 5), 1 / 25, dtype=dtype, device=device)


def test_crop_reproduces_a_local_model_and_feather_does_not():
    """A 5 x 5 box filter with zero padding has radius 2 = v // 2 for v = 4: under `crop` every pixel comes from a tile that
    holds its whole neighbourhood (at the image border the tile's zero padding IS the image's), so the tiled result is the
    whole-image one. `feather` also mixes in the rows a tile computed next to its own zero padding: it must miss the bar,
    which shows that this test can fail."""
    y = image(3, 40, 56, seed=5)
    model = lambda t: F.conv2d(t, box_filter(3, torch.float32, t.device), padding=2, groups=3)
    whole32 = model(y.cuda()[None])[0].cpu()
    whole64 = F.conv2d(y.double()[None], box_filter(3, torch.float64, "cpu"), padding=2, groups=3)[0]
    got = tiling.TiledModel(model, tile=16, overlap=4, batch=4, window="crop")(y.cuda())
    S.hold32("TiledModel crop around a 5x5 box filter", got, whole64, whole32)
    feather = tiling.TiledModel(model, tile=16, overlap=4, batch=4, window="feather")(y.cuda())
    assert S.relerr(feather, whole64) > 100 * S.bar(S.relerr(whole32, whole64))


def test_tiled_upsample_kind_away_from_the_seams():
    """Upsample(factor=2) through TiledModel(scale=2): bicubic taps reach 2 input pixels, so an output pixel farther than 8
    output pixels from every tile edge interior to the image sees in each covering tile what it sees in the image."""
    from models import Upsample
    model = Upsample(factor=2).cuda()
    C, H, W, T, v = 3, 32, 48, 16, 8
    y = image(C, H, W, seed=9)
    got = tiling.TiledModel(model, tile=T, overlap=v, batch=8, scale=2, window="feather")(y.cuda())
    assert got.shape == (3, 64, 96)
    whole32 = model(y.cuda()[None])[0].cpu()
    whole64 = F.interpolate(y.double()[None], scale_factor=2, mode="bicubic", align_corners=False)[0]

    def far(n):
        origins, Te = R.plan(n, T, v)
        edges = {2 * o for o in origins if o > 0} | {2 * (o + Te) for o in origins if o + Te < n}
        return torch.tensor([all(p - e >= 8 if p >= e else e - 1 - p >= 8 for e in edges) for p in range(2 * n)])
    mask = far(H)[:, None] & far(W)[None, :]
    assert bool(mask.any()) and not bool(mask.all())
    S.hold32("TiledModel around Upsample, away from the seams", got[:, mask].cpu(), whole64[:, mask], whole32[:, mask])


def test_mismatching_model_output_names_both_extents():
    extra_row = lambda t: F.pad(t, (0, 0, 0, 1))
    with pytest.raises(ValueError) as err:
        tiling.TiledModel(extra_row, tile=8, overlap=2)(torch.rand(3, 16, 16, device="cuda"))
    message = str(err.value)
    assert "9, 8)" in message and "(8, 8)" in message and "multiple of 16" in message


def test_tiled_forward_has_the_lower_peak_memory():
    """The allocator's counts are deterministic: the peak of the tiled forward (T = 64, one tile per call) of a 256 x 256
    image is strictly below the whole-image forward's."""
    from models import get_model
    from physics import get_physics
    from settings import DefaultArgParser
    args = DefaultArgParser().parse_args(["--device", "cuda", "--task", "deblurring", "--kernel", "Gaussian_R2",
                                          "--ProposedModel__architecture", "Convolutional",
                                          "--ConvolutionalModel__hidden_channels", "8"])
    torch.manual_seed(0)
    model = get_model(args=args, physics=get_physics(args, device="cuda"), device="cuda").to("cuda").eval()
    y = torch.rand((1, 3, 256, 256), device="cuda")
    tiled = tiling.TiledModel(model, tile=64, overlap=16, batch=1)

    def whole(v):
        with torch.no_grad():
            return model(v)
    peaks = {}
    for name, fn in (("tiled", tiled), ("whole", whole)):
        fn(y)                                                # warm-up: code objects, cached matrices and work buffers
    for name, fn in (("tiled", tiled), ("whole", whole)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn(y)
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated()
        assert out.shape == y.shape and bool(torch.isfinite(out).all())
        print(f"{name}: peak {peaks[name]} bytes, {peaks[name] - base} above the {base} allocated before the call")
        del out
    print(f"tiled / whole peak: {peaks['tiled'] / peaks['whole']:.3f}")
    assert peaks["tiled"] < peaks["whole"]


# ------------------------------------------------------------------------------------------------ test.py
from test_eval_metrics_gpu import COMMON, run_test_py  # noqa: E402


def keys(lines):
    return [ln.split(":")[0] for ln in lines]


def test_test_py_tile_prints_the_plain_runs_lines():
    flags = ["--task", "deblurring", "--print_all_metrics"]
    plain = run_test_py(*flags)
    tiled = run_test_py(*flags, "--tile", "32", "--tile_overlap", "8")
    assert keys(tiled) == keys(plain) and "N: 2" in tiled
    assert len([ln for ln in tiled if ln.startswith("METRICS_")]) == 2
    psnr = lambda lines: float([ln for ln in lines if ln.startswith("PSNR:")][0].split()[-1])
    assert math.isfinite(psnr(tiled)) and math.isfinite(psnr(plain))


def folder_command(folder, *flags):
    model_flags = COMMON[COMMON.index("--kernel"):COMMON.index("--indices")]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), "--device", "cuda", "--dataset", str(folder), "--task",
                        "deblurring", *model_flags, *flags], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip().splitlines()


def test_test_py_tile_on_a_folder_of_odd_sized_measurements_and_its_bootstrap(tmp_path):
    from PIL import Image
    folder = tmp_path / "measurements"
    folder.mkdir()
    rng = np.random.default_rng(0)
    sizes = {"a.png": (50, 70), "b.png": (33, 41)}
    for name, (h, w) in sizes.items():
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(folder / name)
    out = tmp_path / "o"
    lines = folder_command(folder, "--tile", "32", "--tile_overlap", "8", "--save_images", "--out_dir", str(out),
                           "--bootstrap", "4", "--bootstrap_batch", "2")
    for name, (h, w) in sizes.items():
        assert Image.open(out / "estimates" / name).size == (w, h)
    assert "EST_N: 2" in lines
    est = float([ln for ln in lines if ln.startswith("EST_PSNR:")][0].split()[-1])
    assert math.isfinite(est)
