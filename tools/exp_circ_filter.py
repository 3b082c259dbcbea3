#!/usr/bin/env python3
"""Device time of sei_circ_filter_sep beside sei_blur_sep_circ (13-tap Gaussian) at the two shapes DESIGN quotes, and the
two floors that follow from the shape.

    python tools/exp_circ_filter.py                       # launches + HIP-event times (run it under rocprofv3, see
                                                          # tools/profile_circ_filter.sh, for the device times)
    python tools/exp_circ_filter.py --summarize TRACE.csv OUT.csv   # per-case medians of a rocprofv3 kernel trace

Every case is WARM + REPS launches of one entry point, in the fixed order of CASES, so the dispatches of a kernel trace
map back to cases by counting. Floors: 8*H*W*planes bytes at 6.3 TB/s (HBM, achievable) and 2*H*W*(H+W)*planes flop at
157.3 TFLOP/s (float32 vector peak)."""
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))

WARM, REPS = 3, 20
SHAPES = [(96, 48, 48), (24, 256, 256)]
CASES = [(shape, what) for shape in SHAPES for what in ("circ A", "circ A_dagger", "blur 13 taps")]
KERNELS = {"circ": "circ_filter_sep_kernel", "blur": "blur_sep_circ_kernel"}
HBM_BYTES_PER_S, F32_FLOP_PER_S = 6.3e12, 157.3e12


def run():
    import torch
    import physics
    ct = physics.CTLikeFilter()
    blur = physics.BlurV2(kernel=physics.get_kernel("Gaussian_R2")[None, None].cuda())
    fns = {"circ A": ct.A, "circ A_dagger": ct.A_dagger, "blur 13 taps": blur.A}
    for (planes, H, W), what in CASES:
        x = torch.rand(planes // 3, 3, H, W, device="cuda")
        fn = fns[what]
        with torch.no_grad():
            for _ in range(WARM):
                fn(x)
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(REPS + 1)]
            ev[0].record()
            for i in range(REPS):
                fn(x)
                ev[i + 1].record()
            torch.cuda.synchronize()
        us = statistics.median(ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(REPS))
        print(f"{what:14s} {planes:3d} x {H} x {W}: {us:8.1f} us per call (HIP events, launch + allocation included)")


def summarize(trace, out):
    rows = list(csv.DictReader(open(trace)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = {k: [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if name in r["Kernel_Name"]]
           for k, name in KERNELS.items()}
    pos = {k: 0 for k in KERNELS}
    with open(out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["entry", "planes", "H", "W", "median_us", "min_us", "hbm_floor_us", "f32_fma_floor_us", "launches"])
        for (planes, H, W), what in CASES:
            k = what.split()[0]
            d = per[k][pos[k] + WARM: pos[k] + WARM + REPS]
            pos[k] += WARM + REPS
            assert len(d) == REPS, (what, len(d))
            hbm = 8.0 * H * W * planes / HBM_BYTES_PER_S * 1e6
            taps = (H + W) if k == "circ" else 26
            fma = 2.0 * H * W * taps * planes / F32_FLOP_PER_S * 1e6
            w.writerow([what, planes, H, W, f"{statistics.median(d) / 1e3:.2f}", f"{min(d) / 1e3:.2f}", f"{hbm:.2f}",
                        f"{fma:.2f}", REPS])
    print(open(out).read())


if __name__ == "__main__":
    if sys.argv[1:2] == ["--summarize"]:
        summarize(sys.argv[2], sys.argv[3])
    else:
        run()
