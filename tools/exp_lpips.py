#!/usr/bin/env python3
"""Device time of metrics.lpips_fn on one image pair (default 1356 x 2040, a DIV2K validation image), whole and per entry
point, beside the float32-matrix floor: 2 M N K summed over the five convolutions of both images against the exact-f32
MFMA rate DESIGN 4.6 quotes (157 TFLOP/s).

    python tools/exp_lpips.py [--H 1356 --W 2040 --batch 1]

Weights are synthetic (randn * sqrt(2 / fan_in)); the time does not depend on them. Each figure is WARM + REPS calls
between two HIP events, back to back on one stream. The per-entry-point figures re-issue the recorded calls of one
evaluation (_native.record_calls), family by family."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))

F32_MFMA_FLOPS = 157e12
LAYERS = ((3, 64, 11, 4, 2, True), (64, 192, 5, 1, 2, True), (192, 384, 3, 1, 1, False), (384, 256, 3, 1, 1, False),
          (256, 256, 3, 1, 1, False))


def timed(fn, warm=3, reps=10):
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=1356)
    ap.add_argument("--W", type=int, default=2040)
    ap.add_argument("--batch", type=int, default=1)
    args = ap.parse_args()
    import torch
    import _native as N
    import metrics

    g = torch.Generator().manual_seed(0)
    conv_w = [torch.randn((co, ci, k, k), generator=g) * math.sqrt(2.0 / (ci * k * k)) for ci, co, k, _, _, _ in LAYERS]
    conv_b = [torch.randn((co,), generator=g) * 0.1 for _, co, _, _, _, _ in LAYERS]
    lin = [torch.rand((1, co, 1, 1), generator=g) for _, co, _, _, _, _ in LAYERS]
    net = metrics.LPIPS(conv_w, conv_b, lin, device="cuda")
    x = torch.rand((args.batch, 3, args.H, args.W), generator=g).cuda()
    x_hat = (x + 0.1 * torch.randn(x.shape, device="cuda")).clamp(0, 1)

    flops, h, w = 0.0, args.H, args.W
    for ci, co, k, s, p, pool in LAYERS:
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        flops += 2.0 * h * w * co * k * k * ci
        if pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    flops *= 2 * args.batch
    floor_us = flops / F32_MFMA_FLOPS * 1e6

    whole = timed(lambda: metrics.lpips_fn(x_hat, x, net))
    print(f"lpips_fn {args.batch} x {args.H} x {args.W}: {whole:.0f} us per call; {flops / 1e9:.1f} GFLOP in the convolutions, "
          f"floor {floor_us:.0f} us at {F32_MFMA_FLOPS / 1e12:.0f} TFLOP/s -> {floor_us / whole:.2f} of the floor rate")

    # One evaluation with its buffers held: the maps and the partial sums (`held`) and the result stay alive while the
    # recorded calls are re-issued one by one on the same pointers.
    N.record_calls(True)
    held = net._maps_gpu(x_hat, x)
    maps, work = held
    out = torch.empty(args.batch, device="cuda")
    for l, m in enumerate(maps):
        N.call("sei_lpips_layer_dist", m[:args.batch].data_ptr(), m[args.batch:].data_ptr(), net._packed[2][l].data_ptr(), l,
               args.batch, args.H, args.W, out.data_ptr(), int(l > 0), work.data_ptr())
    torch.cuda.synchronize()
    log = N.record_calls(False)
    for i, (name, a) in enumerate(log):
        t = timed(lambda: N.call(name, *a))
        layer = a[6] if name == "sei_lpips_conv_relu" else a[2] if name == "sei_lpips_maxpool" else a[3]
        print(f"  {i:2d} {name:22s} layer {layer}: {t:8.1f} us")
    del held, out


if __name__ == "__main__":
    main()
