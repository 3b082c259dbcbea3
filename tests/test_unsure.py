"""UNSURE without a GPU: the flags' refusals (raised before any GPU object exists), the defaults of a namespace that does not
know the options, the host-side refusals of the two entry points, and closed-form anchors of the float64 restatement
(tests/unsure_ref.py) that tests/test_unsure_gpu.py holds the kernels and the loss module to."""
import argparse
import ctypes

import pytest
import torch

import loss_reduction_ref as L
import unsure_ref as U

COMMON = ["--device", "cuda", "--task", "deblurring", "--kernel", "Gaussian_R2", "--dataset", "synthetic", "--out_dir",
          "unused"]
FLAG = "--sure_unknown_noise"


@pytest.mark.parametrize("flags", [
    ["--method", "proposed", "--ProposedLoss__sure_alternative", "r2r"],
    ["--method", "supervised"], ["--method", "css"], ["--method", "noise2inverse"]])
def test_flag_refusals_name_the_flag_and_need_no_gpu(flags):
    """train.main stops in front of get_physics: on a machine without a GPU anything later would raise another error."""
    import train
    with pytest.raises(ValueError, match=FLAG):
        train.main(COMMON + flags + [FLAG])
    import losses
    with pytest.raises(ValueError, match=FLAG):                   # get_loss refuses the same namespace by itself
        losses.get_loss(train.build_parser().parse_args(COMMON + flags + [FLAG]), physics=None)


def test_several_gpus_and_a_bad_momentum_are_refused():
    import losses
    import train
    for method in ("proposed", "sure"):
        a = train.build_parser().parse_args(COMMON + ["--method", method, FLAG])
        losses.check_unsure_args(a)                               # one GPU: accepted
        with pytest.raises(ValueError, match=FLAG):
            losses.check_unsure_args(a, world=2)
    a = train.build_parser().parse_args(COMMON + ["--method", "sure", FLAG, "--unsure_momentum", "1.0"])
    with pytest.raises(ValueError, match="--unsure_momentum"):
        losses.check_unsure_args(a)
    # without the flag nothing is looked at
    losses.check_unsure_args(train.build_parser().parse_args(COMMON + ["--method", "supervised"]), world=8)


def test_parser_defaults():
    import train
    a = train.build_parser().parse_args(COMMON + ["--method", "proposed"])
    assert a.sure_unknown_noise is False and a.unsure_step_size == 1e-4 and a.unsure_momentum == 0.9
    assert a.unsure_init_noise_level is None                      # resolved in get_loss: --noise_level
    b = train.build_parser().parse_args(COMMON + [FLAG, "--unsure_init_noise_level", "12.5", "--no-sure_unknown_noise"])
    assert b.sure_unknown_noise is False and b.unsure_init_noise_level == 12.5


def _namespace(**over):
    """What tests and bench.py hand get_loss: a namespace that has never heard of the UNSURE options."""
    a = argparse.Namespace(partial_sure=True, sure_margin=2, task="deblurring", Loss__crop_training_pairs=True,
                           Loss__crop_size=48, ProposedLoss__stop_gradient=True, ProposedLoss__sure_alternative=None,
                           ProposedLoss__alpha_tradeoff=1.0, ProposedLoss__transforms="Scaling_Transforms",
                           ScalingTransform__kind="padded", ScalingTransform__antialias=False, method="proposed",
                           noise_level=5, sure_cropped_div=True, sure_averaged_cst=False)
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("method", ["proposed", "sure"])
def test_get_loss_without_the_new_attributes_has_unsure_off(method):
    import losses
    loss = losses.get_loss(_namespace(method=method), physics=None)
    term = loss.loss.sure if method == "proposed" else loss.loss.loss
    assert term.unsure is False and loss.unsure_term() is None
    assert not hasattr(term, "noise_state") and dict(loss.named_buffers()) == {}
    assert term.sigma2 == (5 / 255) ** 2
    with pytest.raises(RuntimeError):
        term.estimated_sigma()


@pytest.mark.parametrize("method", ["proposed", "sure"])
def test_get_loss_with_the_flag_builds_the_state_from_the_starting_guess(method):
    import losses
    a = _namespace(method=method, sure_unknown_noise=True, unsure_init_noise_level=15.0, unsure_step_size=3e-4,
                   unsure_momentum=0.5)
    loss = losses.get_loss(a, physics=None)
    term = loss.unsure_term()
    assert term is (loss.loss.sure if method == "proposed" else loss.loss.loss)
    assert (term.step_size, term.momentum) == (3e-4, 0.5)
    assert term.noise_state.dtype == torch.float32
    assert torch.equal(term.noise_state, torch.tensor([(15 / 255) ** 2, 0, 0, 0], dtype=torch.float32))
    assert abs(255 * term.estimated_sigma() - 15) < 1e-5
    assert [n for n, _ in loss.named_buffers() if n.endswith("noise_state")] != []       # what graphs.py restores
    assert loss.loss.graph_safe                                   # unaffected
    # the default starting guess is --noise_level; the state round-trips through state_dict in place
    other = losses.get_loss(_namespace(method=method, sure_unknown_noise=True), physics=None).unsure_term()
    assert float(other.noise_state[0]) == float(L.f32((5 / 255) ** 2))
    address = other.noise_state.data_ptr()
    other.load_state_dict(term.state_dict())
    assert torch.equal(other.noise_state, term.noise_state) and other.noise_state.data_ptr() == address
    with pytest.raises(ValueError, match="momentum"):
        losses.SureGaussianLoss(sigma=0.1, unsure=True, momentum=1.0)


def test_entry_points_refuse_bad_arguments_on_the_host():
    """SEI_ERR_BAD_ARG before any HIP call (fake pointers: a refused call launches nothing and dereferences nothing)."""
    import _native
    lib = _native.lib()
    P, Q = 4096, 4100
    ok = dict(y=P, y1=P, y2=P, b=P, planes=2, H=8, W=6, md=2, mm=2, tau=0.01, c_mse=0.1, inv_n_div=0.1, step=1e-4,
              mu=0.9, update=1, state=P, out3=P, g1=P, g2=P, work=P, stream=None)
    assert len(ok) == len(_native.SIGNATURES["sei_sure_loss_unsure"])
    bad = [dict(state=None), dict(state=Q), dict(state=P + 8), dict(mu=-0.1), dict(mu=1.0), dict(mu=float("nan")),
           dict(step=float("inf")), dict(step=float("-inf")), dict(step=float("nan")), dict(update=2), dict(update=-1),
           dict(md=3), dict(mm=3), dict(H=4), dict(tau=0.0), dict(planes=0), dict(y=None), dict(out3=None), dict(work=None)]
    for change in bad:
        assert lib.sei_sure_loss_unsure(*dict(ok, **change).values()) == 10001, change
    assert lib.sei_axpy_sqrt_dev(None, P, P, P, 4, None) == 10001
    assert lib.sei_axpy_sqrt_dev(P, P, None, P, 4, None) == 10001
    assert lib.sei_axpy_sqrt_dev(P, P, P, P, 0, None) == 10001
    for a, b, out in ((Q, P, P), (P, Q, P), (P, P, Q)):
        assert lib.sei_axpy_sqrt_dev(a, b, P, out, 8, None) == 10001
    assert lib.sei_axpy_sqrt_dev(P, P, P + 2, P, 8, None) == 10001
    assert isinstance(lib, ctypes.CDLL)


# ---------------------------------------------------------------------------------------------- the restatement's own anchors
@pytest.mark.parametrize("mu", [0.0, 0.5, 0.9])
def test_constant_divergence_moves_eta_linearly(mu):
    """A constant d: m is 2 d from the first update on whatever the momentum (mu 2d + (1 - mu) 2d), so
    eta_K = eta_0 + 2 K alpha d."""
    eta0, alpha, d, K = 0.01, 1e-3, -0.37, 25
    eta, m, k = eta0, 0.0, 0
    for _ in range(K):
        eta, m, k = U.ascent(eta, m, k, d, alpha, mu)
        assert abs(m - 2 * d) <= 4e-16
    assert k == K and abs(eta - (eta0 + 2 * K * alpha * d)) <= 1e-15


def test_zero_divergence_leaves_eta_fixed_and_a_stale_m_is_ignored_at_first():
    eta, m, k = 0.02, 0.0, 0
    for _ in range(7):
        eta, m, k = U.ascent(eta, m, k, 0.0, 0.1, 0.9)
    assert (eta, m, k) == (0.02, 0.0, 7)
    assert U.ascent(0.02, 123.0, 0, 0.25, 0.1, 0.9) == (0.02 + 0.1 * 0.5, 0.5, 1)        # k == 0: m' = g
    assert U.ascent(0.02, 1.0, 3, 0.25, 0.1, 0.9)[1] == 0.9 * 1.0 + (1 - 0.9) * 0.5


def test_restated_loss_is_the_reference_loss_with_eta_for_sigma2_and_no_constant():
    """unsure_loss against loss_reduction_ref.sure (anchored to the oracle's sure_loss by tests/test_loss_reduction_ref.py) on
    one of its cases: the same two sums, c_div = 2 eta / n_div, cst = 0; autograd's gradients are the formula's."""
    planes, H, W, md, mm, border_b = case = (3, 48, 48, 6, 6, False)
    y, y1, y2, b = L.sure_inputs(*case)
    eta = float(L.f32(L.SIGMA ** 2))
    c_mse, _, _ = L.sure_constants(planes, H, W, md, mm)
    n_div = planes * (H - 2 * md) * (W - 2 * md)
    ref = L.sure(y, y1, y2, b, md, mm, L.TAU, c_mse, 2 * eta / n_div, 0.0, torch.float64, rounded=False)
    got = U.unsure_loss_and_grads(y, y1, y2, b, md, mm, L.TAU, eta)
    tau32 = float(L.f32(L.TAU))                                   # (unsure_loss rounds tau as the C call does; `sure` here not)
    assert abs(float(got["d"]) * tau32 / L.TAU - float(ref["div"]) / n_div) <= 1e-14 * float(ref["abs_div"]) / n_div
    assert abs(float(got["mse"]) - float(ref["mse"]) * c_mse) <= 1e-14 * float(got["mse"])
    assert abs(float(got["loss"]) - float(ref["loss"])) <= 1e-7 * float(ref["loss_scale"])
    assert float((got["g2"] - ref["g2"]).abs().max()) <= 1e-7 * float(ref["g2"].abs().max())
    assert float((got["g1"] - ref["g1"]).abs().max()) <= 1e-7 * float(ref["g1"].abs().max())


def test_trajectory_carries_the_pre_update_multiplier_in_loss_and_gradients():
    steps = U.trajectory(3, 2, L.TAU, 0.01, 0.05, 0.9)
    eta = U.rounded(0.01)
    for i, s in enumerate(steps):
        y, y1, y2, b = U.trajectory_inputs(i)
        again = U.unsure_loss_and_grads(y, y1, y2, b, 2, 2, L.TAU, eta)
        assert float(again["loss"]) == float(s["loss"]) and torch.equal(again["g2"], s["g2"])
        assert s["k"] == i + 1 and s["eta"] != eta
        eta = s["eta"]
    assert steps[0]["m"] == 2 * float(steps[0]["d"])
