"""Device time of the fine-tuning optimizer step at the default U-Net's bucket size, on one GPU:

  * sei_sgd_fused with the anchor (18 B/element + the coefficient table, followed by sei_sgd_penalty_finish) and without
    (14 B/element), at the library's grid and at capped, looping grids;
  * sei_adam_fused on the same bucket (30 B/element), the comparand for "how close to the copy rate does it get";
  * sei_adam_anchor_fused (optim.FlatAdam with an anchor) with the anchor (34 B/element + the table, followed by the
    finish; also at 8192 looping workgroups) and without (30 B/element), at the library's grid;
  * the literal torch formulations: losses.weights_distance_loss forward + backward over every named parameter and
    torch.optim.SGD.step() / torch.optim.Adam.step().

Each figure is the mean of `--iters` back-to-back launches between two device events, after a warm-up, repeated
`--trials` times with the variants alternating; the floor is bytes / 6.3 TB/s (the float4-copy rate DESIGN.md uses). The
summary at the end gives each variant's median over the trials and its spread (min .. max).

    python tools/exp_sgd.py [--csv profiles/sgd_fused_times.csv]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scale-equivariant-imaging_amd"), ROOT]

import _native as N  # noqa: E402

COPY_RATE = 6.3e12


def timeit(fn, iters):
    fn()
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--literal_iters", type=int, default=3)
    ap.add_argument("--csv", type=str, default=None)
    opt = ap.parse_args()

    import bench
    from losses.weights_distance_loss import WeightsDistanceLoss
    from models import get_model
    from optim import coefficient_table
    args = bench.reference_args("cuda")
    torch.manual_seed(0)
    model = get_model(args, None, "cuda").to("cuda")
    bb = model.get_backbone()
    p, g, sh = bb.flat_params, bb.flat_grads, bb.flat_shadow
    n = p.numel()
    names = len(list(model.named_parameters()))
    print(f"bucket: {n} elements ({n * 4 / 2**30:.2f} GiB float32), {names} named parameters", flush=True)
    g.normal_()
    g.mul_(1e-3)
    anchor = p.clone()
    coef = coefficient_table(model, 1.0).cuda()
    parts = torch.zeros(N.lib().sei_sgd_partials(0, n, 0), dtype=torch.float64, device="cuda")
    pen = torch.zeros((), device="cuda")
    m, v = torch.zeros_like(p), torch.zeros_like(p)

    def sgd(with_anchor, cap):
        def run():
            N.call("sei_sgd_fused", p.data_ptr(), g.data_ptr(), anchor.data_ptr() if with_anchor else None,
                   coef.data_ptr() if with_anchor else None, 0, n, 1e-4, 1.0, sh.data_ptr(),
                   parts.data_ptr() if with_anchor else None, cap)
            if with_anchor:
                N.call("sei_sgd_penalty_finish", parts.data_ptr(), N.lib().sei_sgd_partials(0, n, cap), pen.data_ptr())
        return run

    def adam():
        N.call("sei_adam_fused", p.data_ptr(), g.data_ptr(), 0, m.data_ptr(), v.data_ptr(), n, 1e-4, 0.9, 0.999, 1e-8,
               0.0, 3, 1.0, sh.data_ptr())

    def adam_anchor(with_anchor, cap):
        def run():
            N.call("sei_adam_anchor_fused", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                   anchor.data_ptr() if with_anchor else None, coef.data_ptr() if with_anchor else None, 0, n, 1e-4, 0.9,
                   0.999, 1e-8, 0.0, 3, 1.0, sh.data_ptr(), parts.data_ptr() if with_anchor else None, cap)
            if with_anchor:
                N.call("sei_sgd_penalty_finish", parts.data_ptr(), N.lib().sei_adam_anchor_partials(0, n, cap), pen.data_ptr())
        return run

    variants = [("sei_sgd_fused anchor + finish, library grid", sgd(True, 0), 18 + 1 / 16),
                ("sei_sgd_fused anchor + finish, 8192 workgroups", sgd(True, 8192), 18 + 1 / 16),
                ("sei_sgd_fused anchor + finish, 2048 workgroups", sgd(True, 2048), 18 + 1 / 16),
                ("sei_sgd_fused no anchor, library grid", sgd(False, 0), 14),
                ("sei_adam_fused", adam, 30),
                ("sei_adam_anchor_fused anchor + finish, library grid", adam_anchor(True, 0), 34 + 1 / 16),
                ("sei_adam_anchor_fused anchor + finish, 8192 workgroups", adam_anchor(True, 8192), 34 + 1 / 16),
                ("sei_adam_anchor_fused no anchor, library grid", adam_anchor(False, 0), 30)]
    rows = []
    for trial in range(opt.trials):
        for name, fn, bytes_per in variants:
            t = timeit(fn, opt.iters)
            floor = bytes_per * n / COPY_RATE * 1e3
            rows.append((trial, name, t, floor, floor / t))
            print(f"trial {trial}  {name:56s} {t:7.3f} ms   floor {floor:6.3f} ms   {100 * floor / t:5.1f} % of the copy rate "
                  f"({bytes_per * n / t / 1e9:5.2f} TB/s)", flush=True)
    t = timeit(lambda: N.call("sei_sgd_penalty_finish", parts.data_ptr(), parts.numel(), pen.data_ptr()), opt.iters)
    rows.append((0, f"sei_sgd_penalty_finish alone, {parts.numel()} partial sums", t, 0.0, 0.0))
    print(f"sei_sgd_penalty_finish alone over {parts.numel()} partial sums: {t * 1e3:.1f} us", flush=True)

    # the literal formulation (eager torch, as demo/train.py:258-268 runs it around the loss)
    del m, v
    wd = WeightsDistanceLoss(pretrained_model=model, lambd=1, device="cuda")
    sgd_torch = torch.optim.SGD(model.parameters(), lr=1e-4)

    def literal():
        sgd_torch.zero_grad()
        wd(model).backward()
        sgd_torch.step()

    adam_torch = torch.optim.Adam(model.parameters(), lr=1e-4)

    def literal_adam():
        adam_torch.zero_grad()
        wd(model).backward()
        adam_torch.step()

    for trial in range(opt.trials):
        for name, fn in (("literal torch: penalty forward + backward + torch.optim.SGD", literal),
                         ("literal torch: penalty forward + backward + torch.optim.Adam", literal_adam)):
            t = timeit(fn, opt.literal_iters)
            rows.append((trial, name, t, 0.0, 0.0))
            print(f"trial {trial}  {name}.step(): {t:7.3f} ms per step", flush=True)

    print("\nmedian over the trials (min .. max):")
    for name in dict.fromkeys(r[1] for r in rows):
        ts = sorted(r[2] for r in rows if r[1] == name)
        per = next(r[3] for r in rows if r[1] == name) * COPY_RATE / 1e3      # bytes per launch (0: not a byte count)
        rate = f"   {per / (ts[len(ts) // 2] * 1e-3) / 1e12:5.2f} TB/s" if per else ""
        print(f"  {name:62s} {ts[len(ts) // 2]:8.3f} ms ({ts[0]:.3f} .. {ts[-1]:.3f}){rate}")
    if opt.csv:
        os.makedirs(os.path.dirname(os.path.abspath(opt.csv)), exist_ok=True)
        with open(opt.csv, "w") as f:
            f.write("trial,variant,ms,floor_ms_at_6.3TBps,fraction_of_copy_rate\n")
            for r in rows:
                f.write(f"{r[0]},{r[1]},{r[2]:.4f},{r[3]:.4f},{r[4]:.4f}\n")


if __name__ == "__main__":
    main()
