#!/usr/bin/env python3
"""One denoiser call of the diffusion U-Net (models/diffunet.py, the DiffPIR_DiffUNet baseline's network) at 1 x 256 x 256
and 1 x 512 x 512: device time per kernel family of the "bf16" mode (sei_adm_*) and end to end, beside the float32
composition of the parity mode and DRUNet's call (models/drunet.py) at the same extents; and each (C, C) 3x3 convolution for
C in 128, 256, 512 beside sei_drunet_conv3x3 at the same extents in the same run -- the yardstick: both are the grid_conv
body of csrc/grid_conv.h, so what separates the two columns is the tap index of a non-power-of-two step count, the bias and
the epilogue's traffic.

    python tools/exp_diffunet.py [--csv OUT.csv]

The native calls of one forward are recorded (_native.record_calls) and re-issued family by family, back to back on one
stream between two HIP events, WARM + REPS times; FLOPs are counted from the layer list (2 per multiply-add, interior
pixels only; attention: its two products). Peak: 2.5 PFLOP/s dense bf16 (MFMA). The end-to-end times include the torch glue
(the embedding MLPs, the state and the clamp of the denoiser call). Weights are random at unit scale: timing does not depend
on them, but zero operands would read high."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))

SHAPES = [(1, 256, 256), (1, 512, 512)]
PEAK = 2.5e15
WARM, REPS = 3, 10


def network_flops(B, H, W):
    """{family: FLOPs} of one call from models.diffunet.plan()."""
    from models.diffunet import CH, DOWN, UP, plan
    f = {"conv3x3": 2.0 * 9 * 3 * CH * B * H * W + 2.0 * 9 * CH * 3 * B * H * W, "conv1x1": 0.0, "attention": 0.0}
    h, w = H, W
    for step in plan():
        if step[0] == "rb":
            _, _, cin, cout, how = step
            if how == DOWN:
                h, w = h // 2, w // 2
            elif how == UP:
                h, w = 2 * h, 2 * w
            px = B * h * w
            f["conv3x3"] += 2.0 * 9 * (cin + cout) * cout * px
            if cin != cout:
                f["conv1x1"] += 2.0 * cin * cout * px
        elif step[0] == "attn":
            c, px = step[2], B * h * w
            f["conv1x1"] += 2.0 * 4 * c * c * px
            f["attention"] += 2.0 * 2 * (h * w) * c * px
    return f


def family(name, args):
    if name == "sei_adm_conv":
        return "conv3x3" if args[5] == 9 else "conv1x1"
    return {"sei_adm_gn_stats": "gn_stats", "sei_adm_gn_apply": "gn_apply", "sei_adm_attention": "attention",
            "sei_adm_pack_image": "conv3x3", "sei_adm_tail": "conv3x3"}[name]


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
    from models.diffunet import DiffUNet
    from models.drunet import DRUNet
    torch.manual_seed(0)
    net = DiffUNet()
    for key, p in net.state_dict().items():
        if p.dim() > 1:
            p.copy_(torch.randn(p.shape) * (1.0 / p[0].numel()) ** 0.5 * (0.5 if "out_layers.3" in key or "proj_out" in key else 1))
        else:
            p.copy_(0.1 * torch.randn(p.shape) + (0.0 if key.endswith("bias") else 1.0))
    net = net.cuda().eval()
    drunet = DRUNet()
    for key, p in drunet.state_dict().items():
        fan_in = p.shape[0] if key.startswith("m_up") and p.shape[-1] == 2 else p[0].numel()
        p.copy_(torch.randn(p.shape) * (2.0 / fan_in) ** 0.5 * (0.25 if key.endswith("res.2.weight") else 1.0))
    drunet = drunet.cuda().eval()
    rows = ["what,B,H,W,launches,ms,tflops,fraction_of_peak"]

    def row(what, B, H, W, launches, t, flops=None):
        rows.append(f"{what},{B},{H},{W},{launches},{t * 1e3:.3f}," +
                    (f"{flops / t / 1e12:.1f},{flops / t / PEAK:.3f}" if flops else ","))
        print(rows[-1], flush=True)

    for B, H, W in SHAPES:
        x = torch.rand((B, 3, H, W), device="cuda")
        flops = network_flops(B, H, W)
        net.compute_dtype = "bf16"
        net(x, 0.05)                                                     # buffers and packed weights
        N.record_calls(True)
        out = net(x, 0.05)
        log = N.record_calls(False)
        assert bool(torch.isfinite(out).all())
        for fam in ("conv3x3", "conv1x1", "attention", "gn_stats", "gn_apply"):
            calls = [(n, a) for n, a in log if family(n, a) == fam]
            row(f"bf16 {fam}", B, H, W, len(calls), timed(lambda: [N.call(n, *a) for n, a in calls]), flops.get(fam))
        row("bf16 all launches", B, H, W, len(log), timed(lambda: [N.call(n, *a) for n, a in log]), sum(flops.values()))
        whole = timed(lambda: net(x, 0.05))
        row("bf16 whole call", B, H, W, len(log), whole, sum(flops.values()))
        net.compute_dtype = "f32"
        net(x, 0.05)
        whole32 = timed(lambda: net(x, 0.05), 1, 3)
        row("f32 composition whole call", B, H, W, "", whole32, sum(flops.values()))
        net.compute_dtype = "bf16"
        drunet(x, 0.05)
        row("DRUNet bf16 whole call", B, H, W, "", timed(lambda: drunet(x, 0.05)))
        net._work = {}                                                   # (the kept activations of this shape)
        # the yardstick: one (C, C) convolution at the extents where the network has it, both families in the same run
        for lvl, c in ((0, 128), (2, 256), (4, 512)):
            h, w = H >> lvl, W >> lvl
            R, guard = B * (h + 2) * (w + 2), w + 3
            xg = (torch.randn((R + 2 * guard, c), device="cuda") * 0.5).to(torch.bfloat16)
            yg = torch.zeros_like(xg)
            trunk = torch.zeros((R, c), device="cuda")
            bias = torch.randn(c, device="cuda")
            wt = (torch.randn((c, 9 * c), device="cuda") * (1.0 / (9 * c)) ** 0.5).to(torch.bfloat16)
            fl = 2.0 * 9 * c * c * B * h * w
            t_adm = timed(lambda: N.call("sei_adm_conv", xg[guard:].data_ptr(), wt.data_ptr(), bias.data_ptr(), c, c, 9, B, h, w,
                                         trunk.data_ptr(), trunk.data_ptr(), None), 3, 20)
            t_dr = timed(lambda: N.call("sei_drunet_conv3x3", xg[guard:].data_ptr(), wt.data_ptr(), c, c, B, h, w, 1,
                                        trunk.data_ptr(), None, trunk.data_ptr(), yg[guard:].data_ptr()), 3, 20)
            row(f"sei_adm_conv C={c} {h}x{w}", B, H, W, 1, t_adm, fl)
            row(f"sei_drunet_conv3x3 C={c} {h}x{w}", B, H, W, 1, t_dr, fl)
    if sys.argv[1:2] == ["--csv"]:
        with open(sys.argv[2], "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
