#!/usr/bin/env python3
"""Time of 20 iterations of sei_tv_prox per schedule (tile, iterations per launch k), beside the eager-torch composition
of the same 20 iterations and the traffic floor, at the three shapes DESIGN 4.7 quotes.

    python tools/exp_tv_prox.py [--csv OUT.csv]

Every schedule goes through the per-call arguments of sei_tv_prox_ex, so this runs against libsei_hip.so or the tuning
build alike (SEI_HIP_LIBRARY picks the library). Each case is WARM + REPS calls on preallocated buffers between two HIP
events, back to back on one stream: the time per call includes the gaps between its ceil(20 / k) launches (and the
device-to-device copy where their number is odd), which is what a caller pays. Floor: every launch reads z, x2, u2 and
writes x2, u2 once, 28 bytes per pixel of a plane, at the 8.0 TB/s bench.py --full books HBM traffic against.
Every schedule is also checked against the default one, bit for bit."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))

ITERS, THS = 20, 0.1
SHAPES = [(96, 48, 48), (3, 256, 256), (3, 1356, 2040)]         # planes, H, W (96 = 3 x 32 patches of 48 x 48)
TILES, KS = (64, 32), (1, 2, 4, 5, 10, 20)
HBM_BYTES_PER_S = 8.0e12
TAU, SIGMA, RHO = 0.01, 12.5, 1.99


def eager(z, x2, u2, ths, iters):
    """The same iterations as elementwise and shifted-slice torch operations (what deepinv's TVDenoiser launches)."""
    import torch
    for _ in range(iters):
        adj = torch.zeros_like(x2)
        adj[..., :-1, :] -= u2[0][..., :-1, :]
        adj[..., 1:, :] += u2[0][..., :-1, :]
        adj[..., :, :-1] -= u2[1][..., :, :-1]
        adj[..., :, 1:] += u2[1][..., :, :-1]
        x = (x2 - TAU * adj + TAU * z) / (1 + TAU)
        w = 2 * x - x2
        v = u2.clone()
        v[0][..., :-1, :] += SIGMA * (w[..., 1:, :] - w[..., :-1, :])
        v[1][..., :, :-1] += SIGMA * (w[..., :, 1:] - w[..., :, :-1])
        u = v / torch.clamp(torch.sqrt(v[0] * v[0] + v[1] * v[1]) / ths, min=1.0)
        x2 = x2 + RHO * (x - x2)
        u2 = u2 + RHO * (u - u2)
    return x2, u2


def timed(fn, warm, reps):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def main():
    import torch
    import _native as N
    rows = ["what,planes,H,W,tile,k,launches,us_per_20_iterations,floor_us_per_20_iterations,same_bits_as_default"]
    for planes, H, W in SHAPES:
        g = torch.Generator().manual_seed(planes + H)
        z = torch.rand((planes, H, W), generator=g).cuda()
        x2, u2 = z.clone(), torch.zeros((2, planes, H, W), device="cuda")
        work = torch.empty(N.lib().sei_tv_prox_work_floats(planes, H, W), device="cuda")
        reps = 5 if H * W > 1 << 20 else 20

        def call(tile, k):
            N.call("sei_tv_prox_ex", z.data_ptr(), x2.data_ptr(), u2.data_ptr(), planes, H, W, THS, ITERS, tile, k,
                   work.data_ptr())

        def fresh(tile, k):
            x2.copy_(z)
            u2.zero_()
            call(tile, k)
            return x2.clone(), u2.clone()

        want = fresh(0, 0)
        for tile in TILES:
            for k in KS:
                got = fresh(tile, k)
                same = torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
                launches = -(-ITERS // k)
                us = timed(lambda: call(tile, k), 3, reps)
                floor = launches * 28.0 * planes * H * W / HBM_BYTES_PER_S * 1e6
                rows.append(f"sei_tv_prox,{planes},{H},{W},{tile},{k},{launches},{us:.1f},{floor:.1f},{int(same)}")
                print(rows[-1], flush=True)
        x2.copy_(z)
        u2.zero_()
        ex, eu = eager(z, x2, u2, THS, ITERS)
        err = float((ex - want[0]).abs().max())
        us = timed(lambda: eager(z, x2, u2, THS, ITERS), 1, 3)
        rows.append(f"eager torch (max |x2 - kernel| {err:.1e}),{planes},{H},{W},,,,{us:.1f},,")
        print(rows[-1], flush=True)
    if sys.argv[1:2] == ["--csv"]:
        with open(sys.argv[2], "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
