#!/usr/bin/env python3
"""Device time of blur-then-decimate (physics.BlurDownsampling: sei_blur_decimate, or the banded resampler for rank-1
kernels under replicate / reflect) beside the composition it replaces, on the entry points the tree had before it:

    A      the full-resolution blur, then a strided copy [o::s, o::s]
    A^T    a zero-insert at (o::s, o::s) (a fill and a strided copy), then the full-resolution blur transposed

`dense` runs the composition's blur on sei_blur_dense_circ / sei_blur_dense_pad whatever the kernel; `own route` on what
the deblurring operator itself launches for that kernel (sei_blur_sep_circ or the banded resampler for a rank-1 kernel; the
dense entry points again otherwise). Shapes: 96 planes of 96 x 96 at rate 2 and of 192 x 192 at rate 4 (the training crops),
and one 3 x 1024 x 1024 image at both rates; Gaussian_R1 (7 x 7, rank 1) and a dense 13 x 13; circular and replicate.

    python tools/exp_blur_decimate.py [--out profiles/blur_decimate_times.csv]

Every variant of a case is captured as a hipGraph of CALLS back-to-back calls (so the window is device time, not the
interpreter's enqueue rate), warmed, and then replayed SAMPLES times between HIP events, the variants of a case ALTERNATING
within one process; the csv holds the median per call and the spread (min, max) of those samples. The outputs of the
variants are compared first (max-norm relative, 2e-6)."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))

CALLS, WARM, SAMPLES = 20, 3, 15
SHAPES = [(96, 96, 96, 2), (96, 192, 192, 4), (3, 1024, 1024, 2), (3, 1024, 1024, 4)]      # planes, H, W, rate
KERNELS = ("Gaussian_R1", "dense13x13")
MODES = ("circular", "replicate")


def build_case(torch, N, physics, planes, H, W, rate, kname, mode, transpose):
    """{variant: (fn, out)}: closures on preallocated operands, one call each."""
    from physics._ops import BlurDecimateOp
    if kname == "Gaussian_R1":
        k = physics.get_kernel("Gaussian_R1")
    else:
        k = torch.rand((13, 13), generator=torch.Generator().manual_seed(13), dtype=torch.float64)
        k = k / k.sum()
    kv, kh = k.shape
    phase = 0
    op = BlurDecimateOp(k, rate, mode, phase)
    blur = physics.BlurV2(kernel=k[None, None].cuda()) if mode == "circular" else \
        physics.Blur(filter=k[None, None].cuda(), padding=mode, device="cuda")
    kd = k.float().cuda().contiguous()
    h, w = op.out_length(H), op.out_length(W)
    gen = torch.Generator().manual_seed(planes + H + rate)
    img = torch.rand((planes // 3, 3, H, W), generator=gen).cuda()
    meas = torch.rand((planes // 3, 3, h, w), generator=gen).cuda()
    full = torch.empty_like(img)          # the composition's full-resolution intermediate
    code = {"circular": 0, "replicate": 1}[mode]
    pad_work = None
    if mode != "circular" and transpose:
        pad_work = torch.empty(N.lib().sei_blur_dense_pad_work_floats(planes, H, W, kv, kh, code, 1), device="cuda")

    def dense_blur(src, dst):
        if mode == "circular":
            N.call("sei_blur_dense_circ", src.data_ptr(), dst.data_ptr(), kd.data_ptr(), kv, kh, planes, H, W, int(transpose))
        else:
            N.call("sei_blur_dense_pad", src.data_ptr(), dst.data_ptr(), kd.data_ptr(), kv, kh, planes, H, W, code,
                   int(transpose), N.ptr(pad_work))

    out = {}
    if not transpose:
        y_new, y_dense, y_own = (torch.empty_like(meas) for _ in range(3))

        def new():
            y_new.copy_(op.run(img, False)) if op.route == "bands" else new_kernel(img, y_new)

        def dense():
            dense_blur(img, full)
            y_dense.copy_(full[..., phase::rate, phase::rate])

        def own():
            y_own.copy_(blur._op.run(img, False)[..., phase::rate, phase::rate])
        out = {"new": (new, y_new), "dense": (dense, y_dense), "own route": (own, y_own)}
    else:
        x_new, x_dense, x_own = (torch.empty_like(img) for _ in range(3))
        up = torch.empty_like(img)

        def new():
            x_new.copy_(op.run(meas, True, (H, W))) if op.route == "bands" else new_kernel(meas, x_new)

        def dense():
            up.zero_()
            up[..., phase::rate, phase::rate] = meas
            dense_blur(up, x_dense)

        def own():
            up.zero_()
            up[..., phase::rate, phase::rate] = meas
            x_own.copy_(blur._op.run(up, True))
        out = {"new": (new, x_new), "dense": (dense, x_dense), "own route": (own, x_own)}

    work = None
    floats = N.lib().sei_blur_decimate_work_floats(planes, H, W, kv, kh, code, rate, int(transpose))
    if floats:
        work = torch.empty(floats, device="cuda")

    def new_kernel(src, dst):
        N.call("sei_blur_decimate", src.data_ptr(), dst.data_ptr(), kd.data_ptr(), kv, kh, planes, H, W, code, rate, phase,
               phase, int(transpose), N.ptr(work))

    # (the bands route and the operators' own routes allocate their result and copy it out: one extra small launch, counted)
    return out, op.route


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="csv to write (default: print only)")
    o = ap.parse_args()
    import torch
    import _native as N
    import physics
    if not torch.cuda.is_available():
        raise SystemExit("exp_blur_decimate: needs the GPU (there is no CPU timing of a HIP kernel)")
    rows = []
    for planes, H, W, rate in SHAPES:
        for kname in KERNELS:
            for mode in MODES:
                for transpose in (False, True):
                    variants, route = build_case(torch, N, physics, planes, H, W, rate, kname, mode, transpose)
                    with torch.no_grad():
                        for fn, _ in variants.values():                  # eager first: taps, bands, workspaces, LDS allowance
                            fn()
                        torch.cuda.synchronize()
                        ref = variants["dense"][1].double()
                        errs = {name: float((buf.double() - ref).abs().max() / ref.abs().max())
                                for name, (_, buf) in variants.items()}
                        assert max(errs.values()) < 2e-6, (planes, H, W, rate, kname, mode, transpose, errs)
                        graphs = {}
                        s = torch.cuda.Stream()
                        s.wait_stream(torch.cuda.current_stream())
                        with torch.cuda.stream(s):
                            for name, (fn, _) in variants.items():
                                g = torch.cuda.CUDAGraph()
                                with torch.cuda.graph(g, stream=s):
                                    for _ in range(CALLS):
                                        fn()
                                graphs[name] = g
                        torch.cuda.synchronize()
                        times = {name: [] for name in graphs}
                        for it in range(WARM + SAMPLES):
                            for name, g in graphs.items():               # alternating
                                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                                a.record()
                                g.replay()
                                b.record()
                                b.synchronize()
                                if it >= WARM:
                                    times[name].append(a.elapsed_time(b) * 1e3 / CALLS)
                    row = {"planes": planes, "H": H, "W": W, "rate": rate, "kernel": kname, "padding": mode,
                           "direction": "A^T" if transpose else "A", "new_route": route}
                    for name, t in times.items():
                        key = name.replace(" ", "_")
                        row[f"{key}_median_us"] = f"{statistics.median(t):.2f}"
                        row[f"{key}_min_us"] = f"{min(t):.2f}"
                        row[f"{key}_max_us"] = f"{max(t):.2f}"
                    rows.append(row)
                    print(", ".join(f"{k} {v}" for k, v in row.items()), flush=True)
    if o.out:
        with open(o.out, "w", newline="") as f:
            wr = csv.DictWriter(f, fieldnames=list(rows[0]))
            wr.writeheader()
            wr.writerows(rows)
        print("wrote", o.out)


if __name__ == "__main__":
    main()
