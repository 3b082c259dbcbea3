"""Worker of tests/test_adam_group_step_gpu.py: two replays of a captured proposed-loss step with the optimizer step of the
deepest level's 1x1 weights inside their weight-gradient GEMMs, then one eager step with the same sinks registered (what
bench.py's record_one_step does), on a small U-Net (hidden 32, 3 scales: 512 x 2048 and 2048 x 512 at the deepest level,
whole 128 x 256 tiles). The test runs it twice as a fresh process -- models/_wgrad.py reads SEI_NO_ADAM_GROUP when it is
imported -- and compares what this writes to the file named on the command line, bit for bit.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))
sys.path.insert(1, ROOT)


def main(out_path):
    import bench
    import models
    import physics
    from graphs import GraphedLossStep
    from losses import get_loss
    from models import _ops
    from optim import FlatAdam

    _ops.set_compute_dtype("bf16")
    args = bench.reference_args("cuda", 32, 3)
    torch.manual_seed(0)
    p = physics.get_physics(args, "cuda")
    model = models.get_model(args, p, "cuda").to("cuda")
    bb = model.get_backbone()
    lf = get_loss(args, p)
    opt = FlatAdam(model, lr=3e-4)
    x = torch.rand(2, 3, 256, 256, device="cuda")
    torch.cuda.manual_seed(7)
    y = p(x)
    g = GraphedLossStep(lf, model, opt, (2, 3, 48, 48), fuse_optimizer=True, fuse_min_numel=1 << 20, count_nodes=True)
    registered = {v.data_ptr() for v in g.fused_views}

    def state():
        st = opt.state[bb.flat_params]
        return [bb.flat_params.clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), bb.flat_shadow.clone()]

    def restore(saved, step):
        st = opt.state[bb.flat_params]
        for dst, src in zip((bb.flat_params, st["exp_avg"], st["exp_avg_sq"], bb.flat_shadow), saved):
            dst.copy_(src)
        st["step"] = step
        _ops.weights_updated(bb, plain_shadow_written=True)
        torch.cuda.synchronize()

    initial, step0 = state(), int(opt.state[bb.flat_params]["step"])
    torch.manual_seed(31)
    torch.cuda.manual_seed(32)
    losses, after_replay = [], []
    for _ in range(2):
        losses.append(float(g(x, y)))
        opt.step()
        after_replay.append(state())

    # the eager twin of the captured step from the same start, every GEMM launch recorded: the queue is flushed by the
    # same engine callback
    restore(initial, step0)
    torch.manual_seed(31)
    torch.cuda.manual_seed(32)
    _ops.profile_gemms(True)
    _ops.set_fused_adam(*g.fused_table, owner=bb)
    opt.prepare_step()
    try:
        bb.zero_grad_flat(store_weight_grads=True)
        loss = lf(x=x, y=y, model=model)
        loss.backward()
        launched = _ops.fused_adam_launches(owner=bb)
    finally:
        _ops.set_fused_adam(None, None, owner=bb)
    opt.step()
    records = _ops.profile_gemms(False)
    torch.cuda.synchronize()
    entries = [entry for _, entry, _ in records if entry.startswith("sei_gemm_bf16nt_dw2_adam")]
    group_jobs = [a[1] for _, entry, a in records if entry == "sei_gemm_bf16nt_dw2_adam_group"]
    torch.save({"shapes": sorted(tuple(v.shape) for v in g.fused_views), "kernel_nodes": g.node_counts[0],
                "fused_ranges": [tuple(r) for r in opt._fused_ranges],
                "losses": losses + [float(loss)], "served": launched == registered, "entries": entries,
                "group_jobs": group_jobs, "after_replay_1": [t.cpu() for t in after_replay[0]],
                "after_replay_2": [t.cpu() for t in after_replay[1]], "after_eager": [t.cpu() for t in state()]}, out_path)


if __name__ == "__main__":
    main(sys.argv[1])
