#!/usr/bin/env python3
"""Device time of one Deep Image Prior iteration (forward, data-fit term, backward, Adam) at a 256 x 256 image for the three
tasks, three ways: the captured iteration replayed, the same launches issued eagerly, and the same network as plain torch
modules with autograd and torch.optim.Adam on the same GPU (the comparator).

    python tools/exp_dip.py [--csv OUT.csv] [--size 256] [--iterations 60]

Each figure is the time between two HIP events around `iterations` iterations after a warm-up, divided by their number:
wall time on the device's queue, i.e. kernels plus the gaps between them, which is what a fit of thousands of iterations
pays. (A kernel trace would give the kernel time without the gaps; this tool does not run under a profiler.)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def event_ms(fn):
    import torch
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def ours(op, y, sr_factor, iterations, graph):
    """ms per iteration: a fit of `iterations` minus a fit of 3 (the eager warm-up, set-up and the final forward cancel)."""
    import torch
    from models.dip import DeepImagePrior

    def fit(n):
        model = DeepImagePrior(op, sr_factor=sr_factor, iterations=n, graph=graph)
        torch.manual_seed(0)
        return event_ms(lambda: model(y)), model.last_loss

    fit(4)                                                   # caches of the operator, the allocator
    short, _ = fit(3)
    long, loss = fit(3 + iterations)
    return (long - short) / iterations, loss


def torch_modules(op, y, img_shape, iterations):
    import torch
    from models.dip import ConvDecoderParams
    torch.manual_seed(0)
    net = ConvDecoderParams(img_shape).modules.cuda().train()
    z = torch.randn([32, 16, 16], device="cuda")[None]
    opt = torch.optim.Adam(net.parameters(), lr=5e-3)
    loss = None

    def steps(n):
        nonlocal loss
        for _ in range(n):
            opt.zero_grad()
            loss = ((op.A(net(z)) - y) ** 2).mean()
            loss.backward()
            opt.step()

    steps(5)
    return event_ms(lambda: steps(iterations)) / iterations, float(loss)


def main():
    import torch
    import physics
    size, iterations = arg("--size", 256), arg("--iterations", 60)
    tasks = [
        ("deblurring Gaussian_R2", physics.BlurV2(kernel=physics.get_kernel("Gaussian_R2")[None, None].cuda()), None, size),
        ("sr x2", physics.Downsampling(rate=2, antialias=True), 2, size // 2),
        ("invert_a_tomography_like_filter", physics.CTLikeFilter(), None, size),
    ]
    rows = ["task,image,iterations,graph_ms_per_iteration,eager_ms_per_iteration,torch_ms_per_iteration,"
            "loss_graph,loss_eager,loss_torch"]
    for name, op, sr_factor, n in tasks:
        y = torch.rand((1, 3, n, n), generator=torch.Generator().manual_seed(1)).cuda()
        t0 = time.time()
        g_ms, g_loss = ours(op, y, sr_factor, iterations, True)
        e_ms, e_loss = ours(op, y, sr_factor, iterations, False)
        t_ms, t_loss = torch_modules(op, y, (3, size, size), iterations)
        rows.append(f"{name},{size}x{size},{iterations},{g_ms:.3f},{e_ms:.3f},{t_ms:.3f},{g_loss:.6f},{e_loss:.6f},{t_loss:.6f}")
        print(rows[-1], f"({time.time() - t0:.1f} s)", flush=True)
    if "--csv" in sys.argv:
        with open(arg("--csv", ""), "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
