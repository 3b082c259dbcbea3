#!/usr/bin/env python3
"""Device time of sei_noise_quad_hist (noise_estimation.py) beside a plain device-to-device copy of the same
bytes, the streaming floor of one pass over y.

    python tools/exp_noise_est.py [profiles/noise_est_times.csv]

HIP events around CALLS back-to-back launches on the current stream, after WARM untimed rounds; the median and the minimum
of REPS such rounds, per launch. Shapes: one 2040 x 1356 RGB image (a DIV2K-sized measurement), a training batch of 32 crops
of 48 x 48, and a constant image of the first shape: every quad lands in one counter, the worst contention. The histogram
call accumulates (what NoiseEstimator.add issues: no zeroing launch); the copy reads the bytes and writes them once more, so
a ratio below 1 is possible for a kernel that only reads."""
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))

WARM, REPS, CALLS = 5, 30, 20
CASES = (("noisy image", (1, 3, 1356, 2040), "noisy"), ("training batch", (32, 3, 48, 48), "noisy"),
         ("constant image", (1, 3, 1356, 2040), "constant"))


def timed(fn):
    import torch
    for _ in range(WARM):
        for _ in range(CALLS):
            fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(CALLS):
            fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end) * 1e3 / CALLS)           # us per launch
    return statistics.median(times), min(times)


def main(out):
    import torch
    import _native as N
    from noise_estimation import NoiseEstimator
    torch.manual_seed(0)
    rows = []
    for name, shape, kind in CASES:
        if kind == "constant":
            y = torch.full(shape, 0.5, device="cuda")
        else:
            y = (0.5 + 0.3 * torch.sin(torch.arange(shape[-1], device="cuda") / 40.0)).expand(shape) \
                + (10 / 255) * torch.randn(shape, device="cuda")
            y = y.contiguous()
        est = NoiseEstimator("cuda")
        dst = torch.empty_like(y)
        B, C, H, W = shape
        hist = lambda: N.call("sei_noise_quad_hist", y.data_ptr(), B * C, H, W, est.hist.data_ptr(), 1)
        hist_med, hist_min = timed(hist)
        copy_med, copy_min = timed(lambda: dst.copy_(y))
        quads = B * C * (H // 2) * (W // 2)
        counted = int(est.hist.sum()) // ((WARM + REPS) * CALLS)
        nbytes = 4 * y.numel()
        rows.append([name, "x".join(map(str, shape)), nbytes, f"{hist_med:.2f}", f"{hist_min:.2f}", f"{copy_med:.2f}",
                     f"{copy_min:.2f}", f"{hist_med / copy_med:.2f}", f"{nbytes / hist_med / 1e3:.1f}", quads, counted])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["what", "shape", "bytes_of_y", "hist_median_us", "hist_min_us", "copy_median_us", "copy_min_us",
                    "hist_over_copy", "hist_GB_per_s", "quads", "quads_counted_per_call"])
        w.writerows(rows)
    print(open(out).read())


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "noise_est_times.csv"))
