#!/usr/bin/env python3
"""Device time of one equivariant-bootstrap chunk (bootstrap.EquivariantBootstrap, 8 replicas of 3 x 256 x 384, Gaussian_R2
blur, the small Convolutional U-Net of the tests: 8 hidden channels, 3 scales): the three sei_boot_* kernels beside the
physics and the model call.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o q -- python3 tools/exp_bootstrap.py
    python tools/exp_bootstrap.py --summarize OUT/.../q_kernel_trace.csv profiles/bootstrap_times.csv

One estimate of (WARM + REPS + 1) * 8 replicas in chunks of 8. Every chunk starts with one boot_scale_fwd_kernel dispatch,
so the kernel trace splits into chunks by counting those; the first WARM chunks and the last one (which runs into the
closing torch arithmetic) are dropped. A category's time is the sum of its kernels' device time in one chunk."""
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))

WARM, REPS, BATCH = 2, 10, 8
C, H, W = 3, 256, 384
HBM_PEAK_GBS = 8000.0          # the streaming rate bench.py's roofline_hbm divides by
CATEGORIES = (("sei_boot_scale_fwd", ("boot_scale_fwd_kernel",)),
              ("sei_boot_luma_diff", ("boot_luma_diff_kernel", "boot_luma_sum_kernel")),
              ("sei_boot_pullback_accum", ("boot_pullback_accum_kernel",)),
              ("physics: blur + noise", ("::blur_sep_circ_kernel(", "::axpy_kernel(")))      # (the whole kernel names)
REST = "model call + normal draw"


def run():
    import torch
    from bootstrap import EquivariantBootstrap
    from models import get_model
    from physics import get_physics
    from settings import DefaultArgParser
    args = DefaultArgParser().parse_args(["--device", "cuda", "--task", "deblurring", "--kernel", "Gaussian_R2",
                                          "--ProposedModel__architecture", "Convolutional",
                                          "--ConvolutionalModel__hidden_channels", "8", "--ConvolutionalModel__scales", "3"])
    torch.manual_seed(0)
    op = get_physics(args, device="cuda")
    model = get_model(args=args, physics=op, device="cuda").to("cuda").eval()
    y = op(torch.rand((1, C, H, W), device="cuda"))
    boot = EquivariantBootstrap(op, model, samples=(WARM + REPS + 1) * BATCH, batch=BATCH)
    out = boot(y)
    torch.cuda.synchronize()
    print(f"EST_PSNR {out['est_psnr']:.2f} EST_PSNR_Q90 {out['est_psnr_q90']:.2f} over {out['mse'].numel()} replicas")


def summarize(trace, out):
    rows = list(csv.DictReader(open(trace)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    starts = [i for i, r in enumerate(rows) if "boot_scale_fwd_kernel" in r["Kernel_Name"]]
    assert len(starts) == WARM + REPS + 1, len(starts)
    names = [name for name, _ in CATEGORIES] + [REST]
    per = {name: [] for name in names}
    launches = {name: 0 for name in names}
    for k in range(WARM, WARM + REPS):
        total = {name: 0 for name in names}
        count = {name: 0 for name in names}
        for r in rows[starts[k]:starts[k + 1]]:
            name = next((n for n, keys in CATEGORIES if any(key in r["Kernel_Name"] for key in keys)), REST)
            total[name] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            count[name] += 1
        for name in names:
            per[name].append(total[name])
        launches = count
    floor_us = 7 * 4 * BATCH * H * W / (HBM_PEAK_GBS * 1e9) * 1e6          # 6 floats read, 1 written per pixel
    with open(out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["what", "replicas", "C", "H", "W", "median_us", "min_us", "launches_per_chunk", "chunks",
                    "traffic_floor_us", "floor_over_median"])
        for name in names:
            med = statistics.median(per[name]) / 1e3
            floor = [f"{floor_us:.2f}", f"{floor_us / med:.3f}"] if name == "sei_boot_luma_diff" else ["", ""]
            w.writerow([name, BATCH, C, H, W, f"{med:.2f}", f"{min(per[name]) / 1e3:.2f}", launches[name], REPS] + floor)
    print(open(out).read())


if __name__ == "__main__":
    if sys.argv[1:2] == ["--summarize"]:
        summarize(sys.argv[2], sys.argv[3])
    else:
        run()
