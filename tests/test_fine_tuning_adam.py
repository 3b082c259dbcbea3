"""Fine-tuning with Adam, host side (reference: demo/train.py:157-186 with --fine_tuning --optimizer Adam): the argument
rules of sei_adam_anchor_fused, FlatAdam's checkpoint layout over the `only` parameters against torch.optim.Adam's, and
the combinations FlatAdam refuses. Nothing here needs a GPU."""
import pytest
import torch

import fine_tuning_common as ft

KEYS = ["model.model.conv_last.weight", "model.model.conv_last.bias"]


def test_adam_anchor_entry_points_refuse_bad_arguments_without_launching():
    """The table of test_sgd_entry_points_refuse_bad_arguments_without_launching with the two moments and the step number
    added: NULL, misaligned and empty arguments come back as SEI_ERR_BAD_ARG from the host; the number of partial sums
    is host arithmetic with sei_sgd_partials' values."""
    import _native
    L = _native.lib()
    bad = 10001
    H = (1e-3, 0.9, 0.999, 1e-8, 0.0)                           # lr, beta1, beta2, eps, weight_decay

    def call(p=16, g=16, m=16, v=16, a=None, c=None, lo=0, hi=64, step=1, p16=None, parts=None, cap=0):
        return L.sei_adam_anchor_fused(p, g, m, v, a, c, lo, hi, *H, step, 1.0, p16, parts, cap, None)

    assert call(p=None, g=None, m=None, v=None) == bad
    assert call(g=None) == bad
    assert call(m=None) == bad                                  # NULL moments
    assert call(v=None) == bad
    assert call(m=None, v=None) == bad
    assert call(step=0) == bad and call(step=-1) == bad
    assert call(lo=0, hi=0) == bad                              # empty range
    assert call(lo=64, hi=64) == bad
    assert call(hi=6) == bad                                    # not whole quads
    assert call(p=20) == bad                                    # p not 16-byte aligned
    assert call(g=24) == bad                                    # g not 16-byte aligned
    assert call(m=24) == bad and call(v=20) == bad              # the moments neither
    assert call(p16=4) == bad                                   # bf16 copy: 8 bytes
    assert call(cap=-1) == bad
    assert call(a=16, parts=8) == bad                           # anchor without a table
    assert call(a=16, c=4) == bad                               # ... without partials
    assert call(c=4) == bad                                     # table without an anchor
    assert call(parts=8) == bad                                 # partials without an anchor
    assert call(a=16, c=4, parts=8, hi=96) == bad               # hi % 64 with a table
    assert call(a=16, c=4, parts=8, lo=32, hi=128) == bad       # lo % 64 with a table
    assert call(a=24, c=4, parts=8) == bad                      # anchor misaligned
    assert call(a=16, c=4, parts=12) == bad                     # partials: doubles
    assert call(a=16, c=6, parts=8) == bad                      # table: floats
    cases = [(0, 64, 0), (0, 2048, 0), (0, 2052, 0), (64, 9344, 2), (64, 9344, 0), (0, 6, 0), (64, 64, 0),
             (192, 100224, 0), (0, 1 << 34, 0), (0, 1 << 34, 8192)]
    for lo, hi, cap in cases:
        assert L.sei_adam_anchor_partials(lo, hi, cap) == L.sei_sgd_partials(lo, hi, cap), (lo, hi, cap)
    assert L.sei_adam_anchor_partials(0, 2048, 0) == 1 and L.sei_adam_anchor_partials(0, 2052, 0) == 2
    assert L.sei_adam_anchor_partials(64, 9344, 2) == 2 and L.sei_adam_anchor_partials(64, 9344, 0) == 5
    assert L.sei_adam_anchor_partials(0, 6, 0) == 0 and L.sei_adam_anchor_partials(0, 1 << 34, 0) == 1 << 20


def _moments(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=gen), torch.rand(shape, generator=gen)


def test_flat_adam_state_over_conv_last_only():
    """FlatAdam(only = the conv_last pair, anchor=True): torch.optim.Adam([w, b])'s layout, both ways."""
    from optim import FlatAdam
    model = ft.Nested()
    bb = model.get_backbone()
    pair = [model.get_parameter(k) for k in KEYS]
    opt = FlatAdam(model, lr=1e-3, only=KEYS, anchor=True)
    assert opt.state_dict()["state"] == {}                      # empty before a step, as torch's
    assert opt.state_dict()["param_groups"][0]["params"] == [0, 1]
    assert opt._ranges == sorted((p._sei_bucket_offset, p._sei_bucket_offset + (p.numel() + 63) // 64 * 64) for p in pair)
    assert torch.equal(opt.anchor, bb.flat_params) and opt.anchor.data_ptr() != bb.flat_params.data_ptr()
    K = len(list(model.named_parameters()))
    w = pair[0]
    assert float(opt.coef64[w._sei_bucket_offset // 64]) == pytest.approx(1.0 / (K * w.numel()), rel=1e-6)
    assert opt.last_penalty.dim() == 0 and opt.last_penalty.dtype == torch.float32 and float(opt.last_penalty) == 0.0
    # a state as three steps would leave it: moments in the two ranges, a step count
    st = opt.state[bb.flat_params]
    st["step"] = 3
    filled = {}
    for k, p in enumerate(pair):
        m, v = _moments(p.shape, 60 + k)
        off = p._sei_bucket_offset
        st["exp_avg"][off:off + p.numel()] = m.reshape(-1)
        st["exp_avg_sq"][off:off + p.numel()] = v.reshape(-1)
        filled[k] = (m, v)
    mine = opt.state_dict()
    assert sorted(mine["state"]) == [0, 1]
    for k, p in enumerate(pair):
        assert float(mine["state"][k]["step"]) == 3.0
        assert mine["state"][k]["exp_avg"].shape == p.shape
        assert torch.equal(mine["state"][k]["exp_avg"], filled[k][0])
        assert torch.equal(mine["state"][k]["exp_avg_sq"], filled[k][1])
    # it loads into torch.optim.Adam over the same two tensors, and that optimizer's state loads back
    ref = torch.optim.Adam(pair, lr=1.0)
    ref.load_state_dict(mine)
    assert ref.param_groups[0]["lr"] == 1e-3
    for k, p in enumerate(pair):
        assert float(ref.state[p]["step"]) == 3.0 and torch.equal(ref.state[p]["exp_avg"], filled[k][0])
    back = FlatAdam(model, lr=5e-2, only=KEYS, anchor=True)
    back.load_state_dict(ref.state_dict())
    bst = back.state[bb.flat_params]
    assert bst["step"] == 3 and back.param_groups[0]["lr"] == 1e-3
    assert torch.equal(bst["exp_avg"], st["exp_avg"]) and torch.equal(bst["exp_avg_sq"], st["exp_avg_sq"])
    inside = torch.zeros(bb.flat_params.numel(), dtype=torch.bool)
    for lo, hi in back._ranges:
        inside[lo:hi] = True
    assert not bst["exp_avg"][~inside].any() and not bst["exp_avg_sq"][~inside].any()
    # a state over every parameter of the model is not this optimizer's
    with pytest.raises(ValueError, match="parameters"):
        opt.load_state_dict(torch.optim.Adam(model.parameters(), lr=1e-3).state_dict())


def test_whole_bucket_flat_adam_keeps_its_layout():
    """Without `only` -- with or without an anchor -- the state is torch.optim.Adam(model.parameters())'s, as before."""
    from optim import FlatAdam
    model = ft.Nested()
    params = list(model.parameters())
    ref = torch.optim.Adam(params, lr=1e-3).state_dict()
    ref["param_groups"][0] = {k: ref["param_groups"][0][k] for k in FlatAdam(model, lr=1e-3).state_dict()["param_groups"][0]}
    for anchor in (None, True):
        opt = FlatAdam(model, lr=1e-3, anchor=anchor)
        mine = opt.state_dict()
        assert mine["state"] == {} and mine["param_groups"][0]["params"] == list(range(len(params)))
        assert mine["param_groups"] == ref["param_groups"]
        opt.state[model.get_backbone().flat_params]["step"] = 2
        full = opt.state_dict()["state"]
        assert sorted(full) == list(range(len(params)))
        assert all(full[i]["exp_avg"].shape == p.shape for i, p in enumerate(params))
        torch.optim.Adam(params, lr=1.0).load_state_dict(opt.state_dict())
        assert (opt.anchor is None) == (anchor is None) and float(opt.last_penalty) == 0.0
    plain = FlatAdam(model, lr=1e-3)
    assert plain._ranges is None and plain.coef64 is None        # the step stays sei_adam_fused over the whole bucket


def test_flat_adam_refuses_what_knows_no_penalty():
    from optim import FlatAdam
    model = ft.Nested()
    with pytest.raises(ValueError, match="penalty"):
        FlatAdam(model, anchor=True, reducer=object())
    with pytest.raises(ValueError, match="frozen range"):
        FlatAdam(model, only=KEYS, reducer=object())
    opt = FlatAdam(model, only=KEYS)
    grads = model.get_backbone().flat_grads
    with pytest.raises(ValueError, match="frozen range"):
        opt.fuse_weight_updates([grads[:64].view(8, 8)])
    with pytest.raises(ValueError, match="penalty"):
        FlatAdam(model, anchor=True).fuse_weight_updates([grads[:64].view(8, 8)])
