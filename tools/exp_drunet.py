#!/usr/bin/env python3
"""One DRUNet denoiser call (models/drunet.py, the PlugAndPlay baseline's network) at 1 x 256 x 384 and at 32 x 48 x 48:
device time per U-Net level and achieved TFLOP/s of the fused bf16 family (sei_drunet_*), beside the float32 composition
of the parity mode, and the whole call of either (which for the composition includes its torch glue).

    python tools/exp_drunet.py [--csv OUT.csv]

The entry points are the same in libsei_hip.so and in the tuning build (SEI_HIP_LIBRARY picks the library). The native
calls of one forward are recorded (_native.record_calls) and re-issued level by level, back to back on one stream between
two HIP events, WARM + REPS times; a level's FLOPs are counted from the layer list (2 MACs, interior pixels only: the
border rows that the grid form also computes are overhead, not work). Peak: 2.5 PFLOP/s dense bf16 (MFMA) for the fused
family; the composition's f32 MFMA peak is 157 TFLOP/s. Weights are random at He scale: timing does not depend on them,
but zero operands would read high."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))

SHAPES = [(1, 256, 384), (32, 48, 48)]
NC, NB = (64, 128, 256, 512), 4
PEAK = {"bf16": 2.5e15, "f32": 157.3e12}
WARM, REPS = 3, 10


def level_flops(B, H, W):
    """FLOPs per level (the head and the tail count to level 0, a 2x2 convolution to the level it writes)."""
    f = []
    for lvl, c in enumerate(NC):
        px = B * (H >> lvl) * (W >> lvl)
        convs = 2 * NB * (2 if lvl < 3 else 1)
        flops = convs * 2 * 9 * c * c * px
        if lvl == 0:
            flops += 2 * 9 * 4 * c * px + 2 * 9 * c * 3 * px
        if lvl > 0:
            flops += 2 * 4 * NC[lvl - 1] * c * px                       # down into this level
        if lvl < 3:
            flops += 2 * NC[lvl + 1] * 4 * c * (px // 4)                 # up into this level
        f.append(float(flops))
    return f


def level_of(name, args, B, H, W):
    rows = {B * ((H >> l) + 2) * ((W >> l) + 2): l for l in range(4)}
    pix = {B * (H >> l) * (W >> l): l for l in range(4)}
    by_h = {H >> l: l for l in range(4)}
    if name in ("sei_drunet_head", "sei_drunet_tail", "sei_conv3x3_fwd"):
        return 0
    if name in ("sei_drunet_conv3x3", "sei_drunet_down"):
        return by_h[args[5]]
    if name == "sei_drunet_up":
        return by_h[args[5]] - 1
    if name == "sei_pad_nhwc":
        return by_h[args[3]]
    if name == "sei_unpad_nhwc":
        return by_h[args[4]]
    if name == "sei_gemm_f32_ex":
        M, Nn, K = args[3:6]
        if M in rows:
            return rows[M]
        lvl = pix[M]
        return lvl if lvl > 0 and K == 4 * NC[lvl - 1] else lvl - 1      # down into lvl, else up out of lvl
    raise KeyError(name)


def timed(fn, warm=WARM, reps=REPS):
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
    return start.elapsed_time(stop) * 1e-3 / reps


def main():
    import torch
    import _native as N
    from models.drunet import DRUNet
    torch.manual_seed(0)
    net = DRUNet(NC, NB)
    for key, p in net.state_dict().items():
        fan_in = p.shape[0] if key.startswith("m_up") and p.shape[-1] == 2 else p[0].numel()
        p.copy_(torch.randn(p.shape) * (2.0 / fan_in) ** 0.5 * (0.25 if key.endswith("res.2.weight") else 1.0))
    net = net.cuda().eval()
    rows = ["mode,B,H,W,level,launches,ms,tflops,fraction_of_peak"]
    for B, H, W in SHAPES:
        x = torch.rand((B, 3, H, W), device="cuda")
        flops = level_flops(B, H, W)
        whole = {}
        for mode in ("bf16", "f32"):
            net.compute_dtype = mode
            net(x, 0.05)                                                 # buffers and packed weights
            N.record_calls(True)
            out = net(x, 0.05)
            log = N.record_calls(False)
            assert bool(torch.isfinite(out).all())
            for lvl in range(4):
                calls = [(n, a) for n, a in log if level_of(n, a, B, H, W) == lvl]
                t = timed(lambda: [N.call(n, *a) for n, a in calls])
                rows.append(f"{mode},{B},{H},{W},{lvl},{len(calls)},{t * 1e3:.3f},{flops[lvl] / t / 1e12:.1f},"
                            f"{flops[lvl] / t / PEAK[mode]:.3f}")
                print(rows[-1], flush=True)
            whole[mode] = timed(lambda: net(x, 0.05))
            rows.append(f"{mode},{B},{H},{W},whole call,{len(log)},{whole[mode] * 1e3:.3f},{sum(flops) / whole[mode] / 1e12:.1f},"
                        f"{sum(flops) / whole[mode] / PEAK[mode]:.3f}")
            print(rows[-1], flush=True)
        # one ResBlock convolution (epilogue 1, in place on the trunk) per level and tile: what the default tile rests on
        for lvl, c in enumerate(NC):
            h, w = H >> lvl, W >> lvl
            R, guard = B * (h + 2) * (w + 2), w + 3
            xg = (torch.randn((R + 2 * guard, c), device="cuda") * 0.5).to(torch.bfloat16)
            yg = torch.zeros_like(xg)
            trunk = torch.zeros((R, c), device="cuda")
            wt = (torch.randn((c, 9 * c), device="cuda") * (2.0 / (9 * c)) ** 0.5).to(torch.bfloat16)
            fl = 2.0 * 9 * c * c * B * h * w
            for pb in (0, 1, 2, 4):
                t = timed(lambda: N.call("sei_drunet_conv3x3_ex", xg[guard:].data_ptr(), wt.data_ptr(), c, c, B, h, w, 1,
                                         trunk.data_ptr(), None, trunk.data_ptr(), yg[guard:].data_ptr(), pb), 3, 20)
                rows.append(f"conv3x3 pb={pb},{B},{H},{W},{lvl},1,{t * 1e3:.4f},{fl / t / 1e12:.1f},{fl / t / PEAK['bf16']:.3f}")
                print(rows[-1], flush=True)
        print(f"# {B} x {H} x {W}: {sum(flops) / 1e12:.3f} TFLOP per call; f32 composition / bf16 family = "
              f"{whole['f32'] / whole['bf16']:.2f}", flush=True)
        rows.append(f"ratio f32/bf16,{B},{H},{W},whole call,,{whole['f32'] / whole['bf16']:.2f},,")
        net.compute_dtype = "bf16"
    if sys.argv[1:2] == ["--csv"]:
        with open(sys.argv[2], "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
