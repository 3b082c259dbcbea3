#!/usr/bin/env python3
"""Device time of each BM3D kernel at 3 planes of 256 x 384 (one colour image of the evaluation set's size), beside its
algorithmic bytes and flops: sei_bm3d_match, sei_bm3d_ht and sei_bm3d_wiener with n_max 16 and 32 and with both aggregation
forms (agg 0: a tile's blocks summed in LDS, then one global float atomic per touched pixel; agg 1: every block row added to
global memory), and sei_bm3d_finish.

    python tools/exp_bm3d.py [--csv OUT.csv]

It runs against the product library (SEI_HIP_LIBRARY picks another build of the same ABI). Each case is WARM + REPS calls on
preallocated buffers between two HIP events, back to back on one stream. The filters' times include the memset of the two
accumulation planes that the entry point issues. The planes are smooth-plus-noise images: the groups, and with them the work
of the filters, are what matching finds on them (the mean group size is reported).

Bounds per case: `bytes` the compulsory global traffic (every plane read once, the groups written or read once, the
accumulators written once), `atomic_bytes` what the float atomics add (agg 1: 2 x 4 bytes per pixel of every block of every
group; agg 0: 2 x 4 bytes per touched pixel of every tile's footprint, booked here at the full footprint), `flops` the
multiply-adds counted as two: matching 64 x 3 per candidate, a filter's 2-D DCTs 2 x 2 x 8 x 64 x 2 per block plus the
butterflies. Floors: bytes at 8.0 TB/s, atomic bytes at the 1.3 TB/s chip-wide float-atomic rate."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))

PLANES, H, W = 3, 256, 384
STEP, WINDOW, TILE = 3, 39, 4
HBM_BYTES_PER_S, ATOMIC_BYTES_PER_S = 8.0e12, 1.3e12
WARM, REPS = 3, 20


def timed(fn):
    import torch
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(REPS):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / REPS


def planes():
    import math
    import torch
    g = torch.Generator().manual_seed(0)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    out = []
    for p in range(PLANES):
        im = 0.5 + 0.25 * torch.cos(2 * math.pi * (1.3 + p) * y / H + 0.7 * p) * torch.cos(2 * math.pi * 2.1 * x / W)
        im = im + 0.2 * torch.tanh((x / W - 0.4 - 0.1 * p + 0.3 * (y / H - 0.5)) * 30)
        out.append(im + 0.02 * torch.randn((H, W), generator=g))
    return torch.stack(out).clamp(0, 1).cuda()


def main():
    import torch
    import _native as N
    from models import bm3d as B
    img = planes()
    pilot = (img + 0.005 * torch.randn(img.shape, device="cuda")).clamp(0, 1)
    var = torch.full((PLANES, 64), 0.02 ** 2, device="cuda")
    refs = B.ref_blocks(H, W, STEP)
    n = PLANES * H * W
    work = torch.empty((2, PLANES, H, W), device="cuda")
    out = torch.empty_like(img)
    rows = ["kernel,planes,H,W,n_max,agg,mean_group,us,bytes,atomic_bytes,flops,bytes_floor_us,atomics_floor_us"]

    def row(name, n_max, agg, mean_group, us, nbytes, atomic, flops):
        rows.append(f"{name},{PLANES},{H},{W},{n_max},{agg},{mean_group},{us:.1f},{nbytes:.3e},{atomic:.3e},{flops:.3e},"
                    f"{nbytes / HBM_BYTES_PER_S * 1e6:.2f},{atomic / ATOMIC_BYTES_PER_S * 1e6:.2f}")
        print(rows[-1], flush=True)

    tiles = -(-len(range(0, H - 7, STEP)) // TILE) * -(-len(range(0, W - 7, STEP)) // TILE)      # (about: the last positions)
    footprint = ((TILE - 1) * STEP + WINDOW - 1 + 8) ** 2
    for n_max, tau in ((16, B.TAU_HT), (32, B.TAU_WIENER)):
        pos = torch.empty((PLANES, refs, n_max, 2), dtype=torch.int32, device="cuda")
        counts = torch.empty((PLANES, refs), dtype=torch.int32, device="cuda")

        def match():
            N.call("sei_bm3d_match", img.data_ptr(), PLANES, H, W, STEP, WINDOW, float(tau), n_max, pos.data_ptr(),
                   counts.data_ptr(), None)

        us = timed(match)
        blocks = float(counts.sum())
        mean_group = f"{blocks / (PLANES * refs):.1f}"
        candidates = PLANES * refs * WINDOW * WINDOW
        row("sei_bm3d_match", n_max, "", mean_group, us, 4 * n + PLANES * refs * (n_max * 8 + 4), 0, candidates * 64 * 3)
        flops = blocks * (2 * 2 * 8 * 64 * 2 + 2 * 64 * 2)
        group_bytes = PLANES * refs * (n_max * 8 + 4)
        for agg in (0, 1):
            atomic = 8.0 * (PLANES * tiles * footprint if agg == 0 else blocks * 64)

            def ht():
                N.call("sei_bm3d_ht", img.data_ptr(), var.data_ptr(), pos.data_ptr(), counts.data_ptr(), PLANES, H, W, STEP,
                       n_max, WINDOW, 2.7, agg, work.data_ptr(), None)

            def wiener():
                N.call("sei_bm3d_wiener", img.data_ptr(), pilot.data_ptr(), var.data_ptr(), pos.data_ptr(), counts.data_ptr(),
                       PLANES, H, W, STEP, n_max, WINDOW, agg, work.data_ptr())

            row("sei_bm3d_ht", n_max, agg, mean_group, timed(ht), 4 * n + group_bytes + 8 * n, atomic, flops)
            row("sei_bm3d_wiener", n_max, agg, mean_group, timed(wiener), 8 * n + group_bytes + 8 * n, atomic, 2 * flops)

    def finish():
        N.call("sei_bm3d_finish", work.data_ptr(), out.data_ptr(), PLANES, H, W)

    row("sei_bm3d_finish", "", "", "", timed(finish), 12 * n, 0, n)
    if sys.argv[1:2] == ["--csv"]:
        with open(sys.argv[2], "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
