#!/usr/bin/env python3
"""Device time of the blur with a replicate boundary beside the circular one, at the two shapes DESIGN quotes: a 13-tap
separable Gaussian through the banded resampler beside sei_blur_sep_circ, and a dense 13 x 13 kernel through
sei_blur_dense_pad (forward, and the adjoint's two launches) beside sei_blur_dense_circ.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o q -- python3 tools/exp_blur_pad.py
    python tools/exp_blur_pad.py --summarize OUT/.../q_kernel_trace.csv profiles/blur_pad_times.csv

Every case is WARM + REPS calls of one operator, in the fixed order of CASES, so the dispatches of a kernel trace map back
to cases by counting; a case's time is the sum of the kernels one call launches."""
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))

WARM, REPS = 3, 20
SHAPES = [(96, 48, 48), (24, 256, 256)]
# case -> the kernels one call launches, in order
LAUNCHES = {
    "separable replicate A (bands)": ("resample_sepband_kernel",),
    "separable replicate A^T (bands)": ("resample_sepband_kernel",),
    "separable circular A": ("blur_sep_circ_kernel",),
    "dense 13x13 replicate A": ("blur_dense_pad_kernel",),
    "dense 13x13 replicate A^T": ("blur_dense_pad_kernel", "blur_pad_fold_kernel"),
    "dense 13x13 circular A": ("blur_dense_circ_kernel",),
    "dense 13x13 circular A^T": ("blur_dense_circ_kernel",),
}
CASES = [(shape, what) for shape in SHAPES for what in LAUNCHES]


def run():
    import torch
    import physics
    gauss = physics.get_kernel("Gaussian_R2")[None, None].cuda()
    dense = torch.rand((13, 13), generator=torch.Generator().manual_seed(13), dtype=torch.float64)
    dense = (dense / dense.sum())[None, None].cuda()
    sep_rep = physics.Blur(filter=gauss, padding="replicate", device="cuda")
    sep_circ = physics.BlurV2(kernel=gauss)
    den_rep = physics.Blur(filter=dense, padding="replicate", device="cuda")
    den_circ = physics.BlurV2(kernel=dense)
    assert sep_rep._op.separable and sep_circ._op.separable and not den_rep._op.separable and not den_circ._op.separable
    fns = {"separable replicate A (bands)": sep_rep.A, "separable replicate A^T (bands)": sep_rep.A_adjoint,
           "separable circular A": sep_circ.A, "dense 13x13 replicate A": den_rep.A,
           "dense 13x13 replicate A^T": den_rep.A_adjoint, "dense 13x13 circular A": den_circ.A,
           "dense 13x13 circular A^T": den_circ.A_adjoint}
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
        print(f"{what:32s} {planes:3d} x {H} x {W}: {us:8.1f} us per call (HIP events, launch + allocation included)")


def summarize(trace, out):
    rows = list(csv.DictReader(open(trace)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = sorted({k for ks in LAUNCHES.values() for k in ks})
    per = {name: [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if name in r["Kernel_Name"]]
           for name in names}
    pos = {name: 0 for name in names}
    with open(out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["entry", "planes", "H", "W", "median_us", "min_us", "launches_per_call", "calls"])
        for (planes, H, W), what in CASES:
            total = [0] * REPS
            for name in LAUNCHES[what]:
                d = per[name][pos[name] + WARM: pos[name] + WARM + REPS]
                pos[name] += WARM + REPS
                assert len(d) == REPS, (what, name, len(d))
                total = [a + b for a, b in zip(total, d)]
            w.writerow([what, planes, H, W, f"{statistics.median(total) / 1e3:.2f}", f"{min(total) / 1e3:.2f}",
                        len(LAUNCHES[what]), REPS])
    print(open(out).read())


if __name__ == "__main__":
    if sys.argv[1:2] == ["--summarize"]:
        summarize(sys.argv[2], sys.argv[3])
    else:
        run()
