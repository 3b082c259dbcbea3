"""bench.py's options (CPU): a plain run times the steps and nothing else; --full brings back every other leg;
--dump-outputs writes a bounded, repeatable float32 sample of what the last timed step computed."""
import os

import numpy as np
import pytest
import torch

import bench


def test_plain_run_leaves_every_other_leg_to_full():
    plain = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert (plain.steps, plain.warmup, plain.full) == (7, 2, False)
    assert not (plain.cpu_baseline or plain.profile_gemms or plain.secondary)
    full = bench.parse_args(["--full"])
    assert full.cpu_baseline and full.profile_gemms and full.secondary
    some = bench.parse_args(["--full", "--no-secondary", "--no-cpu-baseline"])     # as the dist1 child runs it
    assert some.profile_gemms and not (some.secondary or some.cpu_baseline)
    assert bench.parse_args(["--profile-gemms"]).profile_gemms


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked(argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def test_dump_outputs_is_a_bounded_repeatable_sample(tmp_path, monkeypatch):
    import types

    from models import get_model
    from optim import FlatAdam
    torch.manual_seed(0)
    model = get_model(bench.reference_args("cpu", hidden=4, scales=5), None, "cpu").to("cpu")   # (.to: the flat bucket)
    opt = FlatAdam(model, lr=1e-4)
    backbone = model.get_backbone()
    st = opt.state[backbone.flat_params]
    g = torch.Generator().manual_seed(3)
    st["exp_avg"].copy_(torch.randn(st["exp_avg"].shape, generator=g))
    st["exp_avg_sq"].copy_(torch.rand(st["exp_avg_sq"].shape, generator=g))
    leg = types.SimpleNamespace(optimizer=opt, backbone=backbone)
    monkeypatch.setattr(bench, "DUMP_ELEMENTS", 1 << 14)         # smaller than the bucket: the sampled branch runs too

    bench.dump_outputs(leg, 0.5, str(tmp_path / "a"), True)
    bench.dump_outputs(leg, 0.5, str(tmp_path / "b"), True)
    bench.dump_outputs(leg, 0.5, str(tmp_path / "c"), False)     # a rank that does not write
    assert not (tmp_path / "c").exists()
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["adam_exp_avg_sample.npy", "adam_exp_avg_sq_sample.npy", "loss.npy", "weights_sample.npy"]
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32 and np.array_equal(a, b)
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [0.5]

    slices = list(opt._slices())
    per_tensor = (1 << 14) // len(slices)
    w = np.load(tmp_path / "a" / "weights_sample.npy")
    assert len(w) == sum(min(p.numel(), per_tensor) for p, _ in slices) <= 1 << 14
    # every tensor in bucket order: a small one whole, a large one sampled from its own values
    pos, whole = 0, 0
    for p, _ in slices:
        values = p.detach().reshape(-1).numpy()
        if p.numel() <= per_tensor:
            assert np.array_equal(w[pos:pos + p.numel()], values)
            whole += 1
        else:
            assert np.isin(w[pos:pos + per_tensor], values).all()
        pos += min(p.numel(), per_tensor)
    assert 0 < whole < len(slices)
    m = np.load(tmp_path / "a" / "adam_exp_avg_sample.npy")
    flat = backbone.flat_params.detach().numpy()
    assert not np.array_equal(m, w) and np.isin(w, flat).all()
