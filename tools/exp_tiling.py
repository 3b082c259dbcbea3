#!/usr/bin/env python3
"""Measurements of tiled inference (tiling.py, sei_tile_gather / sei_tile_blend).

    rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d OUT -o q -- python3 tools/exp_tiling.py
    python tools/exp_tiling.py --summarize OUT profiles/tiling_times.csv
    python tools/exp_tiling.py --swinir [profiles/tiling_swinir.csv]

Without a flag: WARM + REPS rounds on one (3, 2040, 1356) image with T = 256, v = 32 (9 x 6 = 54 tiles), each round one
sei_tile_gather over all tiles, one sei_tile_blend per window over all tiles (finish = 1), and two device-to-device copies:
one of the tile batch's bytes (what the gather reads and writes) and one of half the sum of the tile batch and the image
(so that the copy reads + writes the bytes the blend reads + writes under a window that reads every tile element). The copies
are the floor the kernels are compared against. No counters are collected. --summarize reads the traces of that run (the
kernel trace, and the memory-copy trace when the runtime moved the copies itself) and writes the median and minimum per call
over the last REPS rounds.

--swinir: wall time (a host clock around a call that ends in a synchronise) and peak memory of test.py's forward for SwinIR
(deblurring, --compute_dtype bf16) on one 1024 x 1024 synthetic image: whole-image against --tile 256 --tile_batch 8 and
--tile 128 --tile_batch 32, alternated in one process, ROUNDS rounds after one warm-up call of each."""
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))

WARM, REPS = 3, 10
C, H, W, T, V = 3, 2040, 1356, 256, 32
WINDOWS = ("uniform", "feather", "crop")
ROUNDS = 3


def plan():
    from tiling import tile_plan
    (oy, Th, sy), (ox, Tw, sx) = tile_plan(H, T, V), tile_plan(W, T, V)
    return Th, Tw, sy, sx, len(oy), len(ox)


def run():
    import torch
    import _native as N
    Th, Tw, sy, sx, ny, nx = plan()
    total = ny * nx
    torch.manual_seed(0)
    x = torch.rand((C, H, W), device="cuda")
    tiles = torch.empty((total, C, Th, Tw), device="cuda")
    out = torch.empty((C, H, W), device="cuda")
    half = (tiles.numel() + out.numel()) // 2
    src, dst = torch.rand(tiles.numel(), device="cuda"), torch.empty(tiles.numel(), device="cuda")
    for _ in range(WARM + REPS):
        N.call("sei_tile_gather", x.data_ptr(), tiles.data_ptr(), C, H, W, Th, Tw, sy, sx, ny, nx, 0, total)
        for window in range(3):
            N.call("sei_tile_blend", tiles.data_ptr(), out.data_ptr(), C, H, W, Th, Tw, sy, sx, ny, nx, window, 0, total, 0, 1)
        dst.copy_(src)                                      # the bytes of the tile batch
        dst[:half].copy_(src[:half])                        # half of tile batch + image
        torch.cuda.synchronize()
    err = float((out - x).abs().max())                      # (crop ran last: the identity, up to one rounding)
    print(f"{total} tiles of {Th} x {Tw}; tile batch {4 * tiles.numel()} bytes, image {4 * out.numel()} bytes; "
          f"max |blend(gather(x)) - x| = {err:.2e}")
    assert err < 1e-6


def summarize(folder, out):
    Th, Tw, sy, sx, ny, nx = plan()
    tile_bytes, image_bytes = 4 * ny * nx * C * Th * Tw, 4 * C * H * W
    half_bytes = 4 * ((tile_bytes // 4 + image_bytes // 4) // 2)
    find = lambda pattern: sorted(glob.glob(os.path.join(folder, "**", pattern), recursive=True))
    kernels = [r for f in find("*kernel_trace.csv") for r in csv.DictReader(open(f))]
    copies = [r for f in find("*memory_copy_trace.csv") for r in csv.DictReader(open(f))]
    kernels.sort(key=lambda r: int(r["Start_Timestamp"]))
    copies.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    gathers = [dur(r) for r in kernels if "tile_gather_kernel" in r["Kernel_Name"]]
    blends = [dur(r) for r in kernels if "tile_blend_kernel" in r["Kernel_Name"]]
    assert len(gathers) == WARM + REPS and len(blends) == 3 * (WARM + REPS), (len(gathers), len(blends))
    # the two copies of a round: kernels of the runtime (a copy kernel's name says so) or entries of the memory-copy trace
    copy_kernels = [dur(r) for r in kernels if "copy" in r["Kernel_Name"].lower()]
    copy_entries = [dur(r) for r in copies if "DEVICE_TO_DEVICE" in r.get("Direction", "").upper().replace("MEMORY_COPY_", "")]
    moved = copy_kernels if len(copy_kernels) >= 2 * (WARM + REPS) else copy_entries
    source = "kernel trace" if moved is copy_kernels else "memory-copy trace"
    assert len(moved) >= 2 * (WARM + REPS), (len(copy_kernels), len(copy_entries))
    moved = moved[-2 * (WARM + REPS):]
    rows = {"sei_tile_gather": (gathers[WARM:], 2 * tile_bytes, "copy of the tile batch"),
            "copy of the tile batch": (moved[0::2][WARM:], 2 * tile_bytes, "")}
    for k, name in enumerate(WINDOWS):
        read = tile_bytes if name != "crop" else None       # crop reads about one tile element per pixel
        rows[f"sei_tile_blend {name}"] = (blends[k::3][WARM:], (read or image_bytes) + image_bytes,
                                          "copy of half (tile batch + image)")
    rows["copy of half (tile batch + image)"] = (moved[1::2][WARM:], 2 * half_bytes, "")
    med = {k: statistics.median(v[0]) for k, v in rows.items()}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["what", "C", "H", "W", "T", "v", "tiles", "median_us", "min_us", "bytes_read_plus_written", "GB_per_s",
                    "floor", "floor_over_median", "copies_from"])
        for name, (times, nbytes, floor) in rows.items():
            w.writerow([name, C, H, W, T, V, ny * nx, f"{med[name]:.2f}", f"{min(times):.2f}", nbytes,
                        f"{nbytes / med[name] / 1e3:.0f}", floor, f"{med[floor] / med[name]:.3f}" if floor else "", source])
    print(open(out).read())


def swinir(out):
    import torch
    import _native as N
    from models import _ops as model_ops
    from models import get_model
    from physics import get_physics
    from settings import DefaultArgParser
    from tiling import TiledModel
    args = DefaultArgParser().parse_args(["--device", "cuda", "--task", "deblurring", "--kernel", "Gaussian_R2"])
    model_ops.set_compute_dtype("bf16")
    torch.manual_seed(0)
    op = get_physics(args, device="cuda")
    model = get_model(args=args, physics=op, device="cuda").to("cuda").eval()
    y = op(torch.rand((1, 3, 1024, 1024), device="cuda")).contiguous()

    def whole(v):
        with torch.no_grad():
            return model(v)
    paths = (("whole image", whole), ("--tile 256 --tile_batch 8", TiledModel(model, tile=256, overlap=32, batch=8)),
             ("--tile 128 --tile_batch 32", TiledModel(model, tile=128, overlap=32, batch=32)))
    results, failed = {}, {}
    for name, fn in paths:                                                     # warm-up, and the outputs to compare
        try:
            results[name] = fn(y)
            torch.cuda.synchronize()
        except (N.NativeLibraryError, torch.cuda.OutOfMemoryError) as err:     # a refused extent or too little memory is a
            # finding and its row says so; anything else (a device fault among them) ends the run
            failed[name] = " ".join(str(err).split())[:200]
    paths = tuple(p for p in paths if p[0] in results)
    ref = results.get("whole image")
    diffs = {name: float((r - ref).abs().max()) if ref is not None else float("nan") for name, r in results.items()}
    del results, ref
    times, peaks = {name: [] for name, _ in paths}, {}
    for _ in range(ROUNDS):
        for name, fn in paths:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            start = time.perf_counter()
            r = fn(y)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - start) * 1e3)
            peaks[name] = (torch.cuda.max_memory_allocated(), torch.cuda.max_memory_allocated() - base)
            del r
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["path", "image", "rounds", "median_ms", "min_ms", "max_ms", "peak_bytes", "peak_above_resident_bytes",
                    "max_abs_difference_from_whole"])
        for name, _ in paths:
            t = times[name]
            w.writerow([name, "3x1024x1024", ROUNDS, f"{statistics.median(t):.1f}", f"{min(t):.1f}", f"{max(t):.1f}",
                        peaks[name][0], peaks[name][1], f"{diffs[name]:.3e}"])
        for name, why in failed.items():
            w.writerow([name, "3x1024x1024", 0, "not measured: " + why, "", "", "", "", ""])
    print(open(out).read())


if __name__ == "__main__":
    if sys.argv[1:2] == ["--summarize"]:
        summarize(sys.argv[2], sys.argv[3])
    elif sys.argv[1:2] == ["--swinir"]:
        swinir(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "tiling_swinir.csv"))
    else:
        run()
