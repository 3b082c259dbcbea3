"""The host layer's launch sequence as data: for a list of small U-Net configurations and one small SwinIR, two training
steps are run under `_native.record_calls` and every entry-point call is written as [name, arguments], non-pointer arguments
verbatim, each pointer as null or the ordinal of that address's first appearance in the configuration's trace (job tables
are unfolded field by field, tables of plain integers -- tap offsets -- value by value). Two traces taken on the same machine from two versions of the host code must be equal call for call when a
change claims to leave the launches alone.

    python tools/launch_trace.py --out trace.json                     # record (exit 1 if a required entry point is missing)
    python tools/launch_trace.py --compare a.json b.json              # diff two traces
"""
import argparse
import ctypes
import gc
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))
sys.path.insert(1, ROOT)

# (name, compute dtype, loss, crop, graphed, fused Adam[, early release]). The proposed loss calls the model twice (the joint backward). The
# two "ragged" configurations crop to 36 pixels: pixel counts that are no multiple of 128, so the fused MLP backward takes
# its column-sum branch -- they alone launch sei_colsum_bf16, and they alone have no sei_dwstream_bf16_jobs.
CONFIGS = [(f"{dtype}-{method}-eager", dtype, method, 48, False, False)
           for dtype in ("f32", "bf16", "bf16x3") for method in ("supervised", "proposed")]
CONFIGS += [(f"{dtype}-proposed-graph", dtype, "proposed", 48, True, False) for dtype in ("f32", "bf16", "bf16x3")]
CONFIGS += [("bf16-proposed-graph-fused-adam", "bf16", "proposed", 48, True, True),
            ("bf16-supervised-graph", "bf16", "supervised", 48, True, False),
            ("bf16-supervised-ragged", "bf16", "supervised", 36, False, False),
            ("bf16-proposed-ragged", "bf16", "proposed", 36, False, False),
            # every weight gradient stored, and the event after the two largest recorded inside the captured backward
            ("bf16-proposed-graph-early-release", "bf16", "proposed", 48, True, False, True)]
# the bf16 SwinIR step at the smallest size the token-streaming kernels take, on them and on the tiled GEMMs
SWIN_CONFIGS = [("swinir-bf16-streaming", True), ("swinir-bf16-tiled", False)]

# every one of these must occur somewhere in the whole set: a shrunken configuration must not hide a branch
# (sei_colsum_bf16 stands for the column-sum branch of the fused MLP backward)
REQUIRED = ["sei_mlp_fused_fwd", "sei_mlp_fused_bwd", "sei_gemm_bf16nt", "sei_gemm_bf16nt_ws", "sei_transpose_bf16_many",
            "sei_cast_bf16", "sei_cast_bf16_colsum_parts", "sei_cast_transpose_bf16", "sei_split_bf16x2", "sei_split_bf16x3",
            "sei_dwstream_bf16_jobs", "sei_fold_many", "sei_ln_bwd_res", "sei_dwconv7_ln_fwd", "sei_dwconv7_bwd_weight_ex",
            "sei_sepmap2_packed", "sei_conv3x3_bwd_weight_parts", "sei_colsum_bf16", "sei_tokgrad_bf16_blocks",
            "sei_gemm_bf16nt_dw2_taps", "sei_gemm_bf16nt_dw2", "sei_gemm_bf16nt_dw2_adam"]
REQUIRED_ANY = [("sei_sepmap2_bf16", "sei_sepmap2_small", "sei_sepmap2_big")]
WS_COLSUM_ARG = 16           # sei_gemm_bf16nt_ws: the column-sum destination


def run_config(dtype, method, crop, graphed, fused_adam, early_release=False, batch=2):
    """Two steps of one configuration -> the raw call log (GraphedLossStep: its warm-up and capture included)."""
    import torch
    import _native
    import bench
    from graphs import GraphedLossStep
    from losses import get_loss
    from models import _ops, get_model
    from optim import FlatAdam
    from physics import get_physics
    args = bench.reference_args("cuda:0", hidden=32, scales=3)
    args.method, args.Loss__crop_size = method, crop
    _ops.set_compute_dtype(dtype)
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    physics = get_physics(args, "cuda:0")
    model = get_model(args, physics, "cuda:0")
    model.to("cuda:0").train()
    loss_fn = get_loss(args, physics)
    optimizer = FlatAdam(model, lr=1e-4)
    x = torch.rand((batch, 3, 256, 256), generator=torch.Generator().manual_seed(1234)).to("cuda:0")
    y = physics(x)
    torch.cuda.synchronize()
    _native.record_calls(True)
    try:
        if graphed:
            step = GraphedLossStep(loss_fn, model, optimizer, (batch, 3, crop, crop), fuse_optimizer=fused_adam,
                                   fuse_min_numel=1 << 18, early_release=early_release,
                                   **({"store_min_numel": 0} if early_release else {}))
            if fused_adam and not step.fused_views:
                raise RuntimeError("no weight took the fused Adam epilogue")
            if early_release and step.early_grads is None:
                raise RuntimeError("no early-release range was planned")
        for _ in range(2):
            if graphed:
                step(x, y)
            else:
                optimizer.zero_grad()
                loss_fn(x=x, y=y, model=model).backward()
            optimizer.step()
        torch.cuda.synchronize()
    finally:
        log = _native.record_calls(False)
    return log


def run_swin(streaming):
    """Two bf16 steps of a small SwinIR (2 x 32 x 32: 2048 tokens, stochastic depth on) -> the raw call log."""
    import torch
    import _native
    from models import _ops, _wgrad
    from models.swinir import SwinIR
    from optim import FlatAdam
    from oracle import swinir_path
    depths = (3, 2)
    prev = _ops.set_compute_dtype("bf16")
    _wgrad.TOKEN_STREAMING = streaming
    try:
        torch.manual_seed(11)
        model = SwinIR(upscale=2, upsampler="pixelshuffle", depths=depths, num_heads=(6, 6)).cuda()
        model.train()
        optimizer = FlatAdam(model, lr=1e-4)
        gen = torch.Generator().manual_seed(4)
        x = torch.rand((2, 3, 32, 32), generator=gen).cuda()
        go = torch.randn((2, 3, 64, 64), generator=gen).cuda()
        masks = [None if m is None else tuple(v.cuda() for v in m)
                 for m in swinir_path.draw_drop_masks(2, depths=depths, rate=0.4, generator=gen)]
        torch.cuda.synchronize()
        _native.record_calls(True)
        try:
            for _ in range(2):
                optimizer.zero_grad()
                model(x, drop_masks=masks).backward(go)
                optimizer.step()
            torch.cuda.synchronize()
        finally:
            log = _native.record_calls(False)
    finally:
        _wgrad.TOKEN_STREAMING = True
        _ops.set_compute_dtype(prev)
    return log


def portable(log):
    """The log with every device or host address replaced by the ordinal of its first appearance."""
    import _native
    seen = {}

    def ordinal(address):
        address = getattr(address, "value", address)
        return None if not address else seen.setdefault(int(address), len(seen))

    def field(value, ctype):
        if ctype is ctypes.c_void_p:
            return ordinal(value)
        if issubclass(ctype, ctypes.Array):
            return [field(v, ctype._type_) for v in value]
        return value

    out = []
    for name, args in log:
        row = []
        for k, (a, ctype) in enumerate(zip(args, _native.SIGNATURES[name])):
            if ctype is not ctypes.c_void_p:
                row.append(a)
            elif isinstance(a, ctypes.Array) and issubclass(a._type_, ctypes.Structure):    # a job table: one dict per job
                row.append([{f: field(getattr(job, f), t) for f, t in job._fields_} for job in a])
            elif isinstance(a, ctypes.Array):                  # a table of integers (the tap offsets of a 3x3 convolution)
                row.append(list(a))
            elif name == "sei_zero_ranges" and k == 1:         # (offset, count) pairs behind a host pointer
                row.append(list((ctypes.c_ulonglong * (2 * args[2])).from_address(a.value)))
            else:
                row.append(ordinal(a))
        out.append([name, row])
    return out


def missing_entries(traces):
    calls = [c for t in traces.values() for c in t.get("calls", [])]
    names = {name for name, _ in calls}
    miss = [n for n in REQUIRED if n not in names] + [" | ".join(g) for g in REQUIRED_ANY if not names & set(g)]
    if "sei_gemm_bf16nt_colsum" not in names and not any(n == "sei_gemm_bf16nt_ws" and a[WS_COLSUM_ARG] is not None
                                                         for n, a in calls):
        miss.append("a column-sum GEMM launch")
    return miss


def digest(obj):
    return hashlib.sha256(json.dumps(obj, sort_keys=True).encode()).hexdigest()


def strip_pointers(calls, signatures):
    return [[n, [a for a, t in zip(args, signatures[n]) if t is not ctypes.c_void_p]] for n, args in calls]


def compare(path_a, path_b):
    import _native
    a, b = (json.load(open(p)) for p in (path_a, path_b))
    print(f"{path_a}: sha256 {digest(a)}\n{path_b}: sha256 {digest(b)}")
    bad = 0
    for name in sorted(set(a) | set(b)):
        ca, cb = (t.get(name, {}).get("calls") for t in (a, b))
        if ca is None or cb is None or ca == cb:
            verdict = "equal" if ca is not None and ca == cb else "MISSING or failed on one side"
        elif strip_pointers(ca, _native.SIGNATURES) != strip_pointers(cb, _native.SIGNATURES) or len(ca) != len(cb):
            k = next((i for i, (u, v) in enumerate(zip(ca, cb)) if u != v), min(len(ca), len(cb)))
            verdict = f"DIFFERENT at call {k}: {ca[k:k + 1]} vs {cb[k:k + 1]}"
        else:
            k = next(i for i, (u, v) in enumerate(zip(ca, cb)) if u != v)
            verdict = f"names and non-pointer arguments equal, pointer ordinals differ from call {k}: {ca[k]} vs {cb[k]}"
        bad += verdict != "equal"
        print(f"  {name}: {len(ca or [])} / {len(cb or [])} calls, {verdict}")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--only", help="comma-separated configuration names")
    o = ap.parse_args()
    if o.compare:
        return compare(*o.compare)
    traces = {}
    for name, run, *cfg in [(c[0], run_config, *c[1:]) for c in CONFIGS] + [(c[0], run_swin, *c[1:]) for c in SWIN_CONFIGS]:
        if o.only and name not in o.only.split(","):
            continue
        gc.collect()
        gc.disable()            # (a cycle collection at another moment would free, and re-use, other addresses)
        try:
            traces[name] = {"calls": portable(run(*cfg))}
        except Exception as exc:                                # keep the other configurations' traces
            traces[name] = {"error": f"{type(exc).__name__}: {exc}"}
        finally:
            gc.enable()
        print(name, len(traces[name].get("calls", [])), traces[name].get("error", ""), flush=True)
    with open(o.out, "w") as f:
        json.dump(traces, f)
    miss = [] if o.only else missing_entries(traces)
    print("sha256", digest(traces), "missing:", miss)
    return 1 if miss or any("error" in t for t in traces.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
