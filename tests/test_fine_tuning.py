"""Fine-tuning on measurements, host side (reference: demo/train.py:95-114, 144-186, 245-264 and
src/losses/weights_distance_loss.py): the torch WeightsDistanceLoss against the reference's own values (g17), the
coefficient table that sei_sgd_fused reads, FlatSGD's checkpoint layout against torch.optim.SGD's, and the reference's
assertions on the flags as ValueErrors that need no GPU."""
import numpy as np
import pytest
import torch

import fine_tuning_common as ft


def test_weights_distance_loss_matches_the_reference(golden):
    from losses.weights_distance_loss import WeightsDistanceLoss
    g = golden("g17_weights_distance")
    anchor = ft.Bucket(ft.G17_SHAPES, ft.g17_values(g, "anchor"))
    model = ft.Bucket(ft.G17_SHAPES, ft.g17_values(g, "param"))
    loss = WeightsDistanceLoss(pretrained_model=anchor, lambd=1, device="cpu")(model)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    ref32, ref64 = float(g["loss32"]), float(g["loss64"])
    err = abs(float(loss.detach()) - ref64)
    print(f"weights distance: {float(loss.detach()):.9e} vs float64 {ref64:.9e} (error {err:.2e}, reference float32 error "
          f"{abs(ref32 - ref64):.2e}, bar {ft.penalty_bar(ref32, ref64):.2e})")
    assert err <= ft.penalty_bar(ref32, ref64)
    names = list(ft.G17_SHAPES)
    grads = torch.autograd.grad(loss, [getattr(model, n) for n in names])
    ref = np.concatenate([g[f"f64.penalty_grad.{n}"].reshape(-1) for n in names])
    got = np.concatenate([v.double().numpy().reshape(-1) for v in grads])
    worst = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"weights distance gradients: max-norm relative error {worst:.2e}")
    assert worst <= 1e-6
    # the anchors are copies: moving the pretrained model afterwards does not move them
    wd = WeightsDistanceLoss(pretrained_model=model, lambd=1, device="cpu")
    assert float(wd(model)) == 0.0
    with torch.no_grad():
        model.b0.add_(1.0)
    assert float(wd(model)) == pytest.approx(1.0 / 4, rel=1e-6)


@pytest.mark.parametrize("lambd", [1.0, 0.25])
def test_coefficient_table_of_the_g17_module(golden, lambd):
    from optim import coefficient_table
    g = golden("g17_weights_distance")
    model = ft.Bucket(ft.G17_SHAPES, ft.g17_values(g, "anchor"))
    table = coefficient_table(model, lambd)
    total = model.flat_params.numel()
    assert table.dtype == torch.float32 and table.device.type == "cpu"
    assert total % 64 == 0 and table.shape == (total // 64,)
    assert total == 192 + 64 + 2048 + 128                     # 135, 1, 2048 and 65 elements in whole 64-blocks
    covered = torch.zeros(total // 64, dtype=torch.bool)
    K = len(ft.G17_SHAPES)
    for name, p in model.named_parameters():
        lo, n = p._sei_bucket_offset, p.numel()
        assert lo % 64 == 0
        blocks = slice(lo // 64, (lo + n + 63) // 64)
        assert torch.all(table[blocks] == np.float32(lambd / (K * n))), name
        assert not covered[blocks].any()
        covered[blocks] = True
    assert covered.all()


def _sgd_state(params, lr):
    return torch.optim.SGD(params, lr=lr).state_dict()


def test_flat_sgd_state_is_torch_sgd_state():
    from optim import FlatSGD
    model = ft.Nested()
    opt = FlatSGD(model, lr=1e-2)
    ref = _sgd_state(model.parameters(), 1e-2)
    mine = opt.state_dict()
    assert mine["state"] == {} == ref["state"]
    assert mine["param_groups"] == ref["param_groups"]
    assert mine["param_groups"][0]["params"] == list(range(len(list(model.parameters()))))
    # each loads into the other, and a scheduler drives both through param_groups[0]["lr"]
    torch.optim.SGD(model.parameters(), lr=3e-3).load_state_dict(mine)
    other = _sgd_state(model.parameters(), 5e-3)
    opt.load_state_dict(other)
    assert opt.param_groups[0]["lr"] == 5e-3 and opt.state_dict()["param_groups"] == other["param_groups"]
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1], gamma=0.5)
    sched.step()
    assert opt.param_groups[0]["lr"] == 2.5e-3
    assert opt.state_dict()["param_groups"][0]["initial_lr"] == 5e-3
    # what the fused step cannot continue is refused with a message
    p = [torch.nn.Parameter(torch.zeros(3)) for _ in model.parameters()]
    momentum = torch.optim.SGD(p, lr=1e-2, momentum=0.9)
    for q in p:
        q.grad = torch.ones(3)
    momentum.step()
    with pytest.raises(ValueError, match="momentum"):
        opt.load_state_dict(momentum.state_dict())
    for kw in ({"momentum": 0.9, "nesterov": True}, {"maximize": True}, {"weight_decay": 1e-4}):
        with pytest.raises(ValueError):
            opt.load_state_dict(torch.optim.SGD(p, lr=1e-2, **kw).state_dict())
    with pytest.raises(ValueError, match="parameters"):
        opt.load_state_dict(_sgd_state(p[:2], 1e-2))


def test_flat_sgd_state_over_conv_last_only():
    """`only` = the two tensors demo/train.py:180-184 passes to the optimizer, on the project's own SwinIR."""
    import train
    from models import get_model
    from optim import FlatSGD
    a = train.build_parser().parse_args(["--task", "sr", "--sr_factor", "2", "--method", "proposed", "--out_dir", "o"])
    torch.manual_seed(0)
    model = get_model(a, physics=None, device="cpu")
    bb = model.get_backbone()
    bb.flatten_parameters()                                   # what .to(device) does
    pair = [model.get_parameter(k) for k in train.FINE_TUNING_PARAMS]
    opt = FlatSGD(model, lr=1e-2, anchor=True, only=train.FINE_TUNING_PARAMS)
    ref = _sgd_state(pair, 1e-2)
    assert opt.state_dict() == ref and ref["param_groups"][0]["params"] == [0, 1]
    torch.optim.SGD(pair, lr=1.0).load_state_dict(opt.state_dict())
    opt.load_state_dict(_sgd_state(pair, 4e-3))
    assert opt.param_groups[0]["lr"] == 4e-3
    with pytest.raises(ValueError, match="parameters"):
        opt.load_state_dict(_sgd_state(model.parameters(), 1e-2))
    # the step covers the two parameters' own whole 64-blocks and nothing else; K counts every named parameter
    assert opt._ranges == sorted((p._sei_bucket_offset, p._sei_bucket_offset + (p.numel() + 63) // 64 * 64) for p in pair)
    K = len(list(model.named_parameters()))
    w = pair[0]
    assert float(opt.coef64[w._sei_bucket_offset // 64]) == np.float32(1.0 / (K * w.numel()))
    assert torch.equal(opt.anchor, bb.flat_params) and opt.anchor.data_ptr() != bb.flat_params.data_ptr()


def test_sgd_entry_points_refuse_bad_arguments_without_launching():
    """NULL, misaligned and empty arguments come back as SEI_ERR_BAD_ARG from the host (safe without a GPU); the number
    of partial sums is host arithmetic."""
    import _native
    L = _native.lib()
    bad = 10001
    assert L.sei_sgd_fused(None, None, None, None, 0, 64, 0.01, 1.0, None, None, 0, None) == bad
    assert L.sei_sgd_fused(16, None, None, None, 0, 64, 0.01, 1.0, None, None, 0, None) == bad
    assert L.sei_sgd_fused(16, 16, None, None, 0, 0, 0.01, 1.0, None, None, 0, None) == bad          # empty range
    assert L.sei_sgd_fused(16, 16, None, None, 64, 64, 0.01, 1.0, None, None, 0, None) == bad
    assert L.sei_sgd_fused(16, 16, None, None, 0, 6, 0.01, 1.0, None, None, 0, None) == bad          # not whole quads
    assert L.sei_sgd_fused(20, 16, None, None, 0, 64, 0.01, 1.0, None, None, 0, None) == bad         # p not 16-byte aligned
    assert L.sei_sgd_fused(16, 24, None, None, 0, 64, 0.01, 1.0, None, None, 0, None) == bad         # g not 16-byte aligned
    assert L.sei_sgd_fused(16, 16, None, None, 0, 64, 0.01, 1.0, 4, None, 0, None) == bad            # bf16 copy: 8 bytes
    assert L.sei_sgd_fused(16, 16, None, None, 0, 64, 0.01, 1.0, None, None, -1, None) == bad
    assert L.sei_sgd_fused(16, 16, 16, None, 0, 64, 0.01, 1.0, None, 8, 0, None) == bad              # anchor without a table
    assert L.sei_sgd_fused(16, 16, 16, 4, 0, 64, 0.01, 1.0, None, None, 0, None) == bad              # ... without partials
    assert L.sei_sgd_fused(16, 16, None, 4, 0, 64, 0.01, 1.0, None, None, 0, None) == bad            # table without an anchor
    assert L.sei_sgd_fused(16, 16, 16, 4, 0, 96, 0.01, 1.0, None, 8, 0, None) == bad                 # hi % 64 with a table
    assert L.sei_sgd_fused(16, 16, 16, 4, 32, 128, 0.01, 1.0, None, 8, 0, None) == bad               # lo % 64 with a table
    assert L.sei_sgd_fused(16, 16, 24, 4, 0, 64, 0.01, 1.0, None, 8, 0, None) == bad                 # anchor misaligned
    assert L.sei_sgd_fused(16, 16, 16, 4, 0, 64, 0.01, 1.0, None, 12, 0, None) == bad                # partials: doubles
    assert L.sei_sgd_penalty_finish(None, 1, None, None) == bad
    assert L.sei_sgd_penalty_finish(8, 0, 8, None) == bad
    assert L.sei_sgd_penalty_finish(12, 1, 8, None) == bad
    # one workgroup per 2 x 256 quads, capped: 2048 elements per workgroup and trip
    assert L.sei_sgd_partials(0, 64, 0) == 1 and L.sei_sgd_partials(0, 2048, 0) == 1 and L.sei_sgd_partials(0, 2052, 0) == 2
    assert L.sei_sgd_partials(64, 9344, 2) == 2 and L.sei_sgd_partials(64, 9344, 0) == 5
    assert L.sei_sgd_partials(0, 6, 0) == 0 and L.sei_sgd_partials(64, 64, 0) == 0


COMMON = ["--device", "cuda", "--task", "deblurring", "--kernel", "Gaussian_R2", "--out_dir", "unused"]


@pytest.mark.parametrize("flags,message", [
    (["--dataset", "<dir>", "--method", "proposed"], "only supported for fine-tuning"),
    (["--dataset", "<dir>", "--method", "sure", "--fine_tuning"], "proposed method"),
    (["--dataset", "synthetic", "--method", "proposed", "--fine_tuning_params"], "Fine-tuning parameters"),
    (["--dataset", "synthetic", "--method", "proposed", "--weights_distance_loss"], "Weights distance loss"),
    (["--dataset", "synthetic", "--method", "proposed", "--fine_tuning", "--fine_tuning_params",
      "--ProposedModel__architecture", "Convolutional"], "conv_last")])
def test_fine_tuning_flag_checks_need_no_gpu(tmp_path, flags, message):
    import train
    flags = [str(tmp_path) if f == "<dir>" else f for f in flags]
    with pytest.raises(ValueError, match=message):
        train.main(COMMON + flags)


def test_fine_tuning_defaults_are_the_reference_s():
    import train
    a = train.build_parser().parse_args(COMMON + ["--fine_tuning"])
    assert a.lr is None and a.optimizer is None and a.fused_optimizer       # resolved in main(): 1e-2 and SGD
    train.check_fine_tuning_args(a)
    assert train.FINE_TUNING_PARAMS == ["model.model.conv_last.weight", "model.model.conv_last.bias"]
