#!/usr/bin/env python3
"""The DiffPIR_DRUNet baseline (models/diffpir.py) on one 1 x 3 x 256 x 384 deblurring measurement (Gaussian_R2, noise
5 / 255): time per image and per data step with the fused conjugate-gradient kernels (fused_cg=True: sei_cg_*,
sei_diffpir_sample) beside the literal torch path (fused_cg=False), and the denoiser's share of the time.

    python tools/exp_diffpir.py [--iterations N] [--csv OUT.csv]

An image is timed on the wall clock around a synchronised forward (the host reads of either path are part of what is
compared), 1 warm-up and REPS forwards with the same noise, each timed on its own: the median is reported, and the minimum
beside it. The denoiser alone is timed between two HIP events, back
to back at the same extent; "per prox" is what is left of the image, divided by the number of data steps: the conjugate
gradients, the sampling step and their host work. Weights are random at He scale: timing does not depend on them, and the
conjugate-gradient iteration counts depend on the denoiser's output only through the right-hand side."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))

SHAPE = (1, 3, 256, 384)
REPS = 7


def main():
    import torch
    import physics
    from models.diffpir import DiffPIR
    from models.drunet import DRUNet
    argv = sys.argv[1:]
    iterations = int(argv[argv.index("--iterations") + 1]) if "--iterations" in argv else 100
    torch.manual_seed(0)
    net = DRUNet()
    for key, p in net.state_dict().items():
        fan_in = p.shape[0] if key.startswith("m_up") and p.shape[-1] == 2 else p[0].numel()
        p.copy_(torch.randn(p.shape) * (2.0 / fan_in) ** 0.5 * (0.25 if key.endswith("res.2.weight") else 1.0))
    net = net.cuda().eval()
    op = physics.BlurV2(kernel=physics.get_kernel("Gaussian_R2")[None, None].cuda())
    op.noise_model = physics.GaussianNoise(sigma=5 / 255)
    y = op(torch.rand(SHAPE, device="cuda"))
    noise = [torch.randn(SHAPE, device="cuda") for _ in range(iterations + 1)]

    class Fixed(DiffPIR):
        def draw(self, i, like):
            return noise[i]

    x = torch.rand(SHAPE, device="cuda")
    for _ in range(3):
        net(x, 0.05)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(20):
        net(x, 0.05)
    stop.record()
    torch.cuda.synchronize()
    t_net = start.elapsed_time(stop) * 1e-3 / 20
    print(f"denoiser call at {SHAPE}: {t_net * 1e3:.3f} ms", flush=True)

    rows = ["path,iterations,proxes,mean_cg_iterations,ms_per_image_median,ms_per_image_min,ms_per_prox,denoiser_share"]
    for fused in (True, False):
        model = Fixed(op, net, max_iter=iterations, fused_cg=fused)
        model(y)
        torch.cuda.synchronize()
        times = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            out = model(y)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        t = sorted(times)[REPS // 2]                                   # per-prox time and share: from the median image
        assert bool(torch.isfinite(out).all())
        proxes = len(model.cg_iterations)
        rows.append(f"{'fused' if fused else 'literal'},{iterations},{proxes},{sum(model.cg_iterations) / proxes:.1f},"
                    f"{t * 1e3:.1f},{min(times) * 1e3:.1f},{(t - iterations * t_net) / proxes * 1e3:.3f},{iterations * t_net / t:.3f}")
        print(rows[-1], flush=True)
    if "--csv" in argv:
        with open(argv[argv.index("--csv") + 1], "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
