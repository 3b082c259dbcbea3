"""Poisson-Gaussian UNSURE without a GPU: closed-form anchors of the float64 restatement (tests/unsure_pg_ref.py) that
tests/test_unsure_pg_gpu.py holds the kernels and the loss module to, the flags' refusals (raised before any GPU object
exists), the defaults of a namespace that does not know the options, the host-side refusals of the two entry points, and
get_physics' choice of the noise model."""
import argparse

import pytest
import torch

import loss_reduction_ref as L
import unsure_pg_ref as P
import unsure_ref as U

COMMON = ["--device", "cuda", "--task", "deblurring", "--kernel", "Gaussian_R2", "--dataset", "synthetic", "--out_dir",
          "unused"]
FLAG, MODEL = "--sure_unknown_noise", "--unsure_noise_model"
PG = [FLAG, MODEL, "poisson_gaussian"]


# ---------------------------------------------------------------------------------------------- the restatement's own anchors
@pytest.mark.parametrize("md,mm", [(0, 0), (2, 2), (3, 1)])
def test_a_linear_model_has_closed_form_divergences_and_gradient(md, mm):
    """y1 = a y and y2 = a (y + tau b): b (y2 - y1) / tau = a b^2, so d0 = a mean(b^2), d1 = a mean(y b^2) over the
    divergence interior, and d loss / d y2 = 2 (eta + gamma y) b / (tau n_div) there, zero outside. tau = 2^-7 is a float32
    value, so the restatement's rounding of it changes nothing."""
    shape, a, tau, eta, gamma = (2, 3, 12, 10), 0.7, 2.0 ** -7, 0.01, 0.03
    gen = torch.Generator().manual_seed(5)
    y = torch.rand(shape, generator=gen, dtype=torch.float64)
    b = torch.randn(shape, generator=gen, dtype=torch.float64)
    y1, y2 = a * y, a * (y + tau * b)
    r = P.pg_loss_and_grads(y, y1, y2, b, md, mm, tau, eta, gamma)
    in_d, in_m = L.interior(12, 10, md), L.interior(12, 10, mm)
    n_div = 2 * 3 * int(in_d.sum())
    d0, d1 = a * (b ** 2)[..., in_d].mean(), a * (y * b ** 2)[..., in_d].mean()
    assert abs(float(r["d0"]) - float(d0)) <= 1e-12 * float(d0)
    assert abs(float(r["d1"]) - float(d1)) <= 1e-12 * float(d1)
    assert float(r["abs_d0"]) == float(r["d0"]) and float(r["abs_d1"]) == float(r["d1"])      # all terms positive
    mse = ((a - 1) ** 2 * y ** 2)[..., in_m].mean()
    assert abs(float(r["loss"]) - float(mse + 2 * (eta * d0 + gamma * d1))) <= 1e-13
    g2 = torch.where(in_d, 2 * (eta + gamma * y) * b / (tau * n_div), torch.zeros((), dtype=torch.float64))
    assert float((r["g2"] - g2).abs().max()) <= 1e-13 * float(g2.abs().max())
    n_mse = 2 * 3 * int(in_m.sum())
    g1 = torch.where(in_m, 2 * (y1 - y) / n_mse, torch.zeros((), dtype=torch.float64)) - g2
    assert float((r["g1"] - g1).abs().max()) <= 1e-13 * float(g1.abs().max())


def test_gamma_zero_is_the_gaussian_restatement():
    y, y1, y2, b = U.trajectory_inputs(0)
    pg = P.pg_loss_and_grads(y, y1, y2, b, 2, 2, L.TAU, 0.0123, 0.0)
    g = U.unsure_loss_and_grads(y, y1, y2, b, 2, 2, L.TAU, 0.0123)
    assert float(pg["loss"]) == float(g["loss"]) and float(pg["d0"]) == float(g["d"])
    assert torch.equal(pg["g1"], g["g1"]) and torch.equal(pg["g2"], g["g2"])


def test_three_ascent_steps_by_hand():
    """alpha_eta = 0.5, alpha_gamma = 0.25, mu = 0.5 (all exact in binary) from (eta, gamma) = (1, 2):
        step 1 (k = 0: m' = g)   d = (0.25, -0.5)   m = (0.5, -1)        eta = 1.25     gamma = 1.75
        step 2                   d = (0.75, 0.5)    m = (1, 0)           eta = 1.75     gamma = 1.75
        step 3                   d = (-1, 1)        m = (-0.5, 1)        eta = 1.5      gamma = 2"""
    state = (1.0, 0.0, 2.0, 0.0, 0)
    state = P.ascent(state, 0.25, -0.5, 0.5, 0.25, 0.5)
    assert state == (1.25, 0.5, 1.75, -1.0, 1)
    state = P.ascent(state, 0.75, 0.5, 0.5, 0.25, 0.5)
    assert state == (1.75, 1.0, 1.75, 0.0, 2)
    state = P.ascent(state, -1.0, 1.0, 0.5, 0.25, 0.5)
    assert state == (1.5, -0.5, 2.0, 1.0, 3)
    # a stale direction is ignored while k == 0, for both multipliers
    assert P.ascent((1.0, 9.0, 2.0, -9.0, 0), 0.25, -0.5, 0.5, 0.25, 0.5) == (1.25, 0.5, 1.75, -1.0, 1)


def test_trajectory_carries_the_pre_update_multipliers():
    steps = P.trajectory(3, 2, L.TAU, 0.01, 0.03, 0.05, 0.02, 0.9)
    eta, gamma = U.rounded(0.01), U.rounded(0.03)
    for i, s in enumerate(steps):
        y, y1, y2, b = U.trajectory_inputs(i)
        again = P.pg_loss_and_grads(y, y1, y2, b, 2, 2, L.TAU, eta, gamma)
        assert float(again["loss"]) == float(s["loss"]) and torch.equal(again["g2"], s["g2"])
        assert s["k"] == i + 1 and s["eta"] != eta and s["gamma"] != gamma
        eta, gamma = s["eta"], s["gamma"]
    assert steps[0]["m_eta"] == 2 * float(steps[0]["d0"]) and steps[0]["m_gamma"] == 2 * float(steps[0]["d1"])


# ---------------------------------------------------------------------------------------------- flags
def test_parser_defaults():
    import train
    a = train.build_parser().parse_args(COMMON + ["--method", "proposed"])
    assert a.unsure_noise_model == "gaussian" and a.unsure_init_gain == 0.0 and a.unsure_gain_step_size is None
    assert a.noise_gain == 0.0
    b = train.build_parser().parse_args(COMMON + PG + ["--unsure_init_gain", "0.02", "--unsure_gain_step_size", "3e-5",
                                                       "--noise_gain", "0.01"])
    assert (b.unsure_noise_model, b.unsure_init_gain, b.unsure_gain_step_size, b.noise_gain) == \
        ("poisson_gaussian", 0.02, 3e-5, 0.01)
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(COMMON + [MODEL, "poisson"])


def test_the_model_without_the_flag_is_refused_by_name_and_needs_no_gpu():
    """train.main stops in front of get_physics: on a machine without a GPU anything later would raise another error."""
    import losses
    import train
    flags = ["--method", "proposed", MODEL, "poisson_gaussian"]
    with pytest.raises(ValueError, match=MODEL) as e:
        train.main(COMMON + flags)
    assert FLAG in str(e.value)
    with pytest.raises(ValueError, match=MODEL):
        losses.get_loss(train.build_parser().parse_args(COMMON + flags), physics=None)


def test_no_stop_gradient_is_refused_by_its_flag_name():
    import losses
    import train
    flags = ["--method", "proposed", "--no-ProposedLoss__stop_gradient"] + PG
    with pytest.raises(ValueError, match="--no-ProposedLoss__stop_gradient") as e:
        train.main(COMMON + flags)
    assert MODEL in str(e.value)
    with pytest.raises(ValueError, match="--no-ProposedLoss__stop_gradient"):
        losses.get_loss(train.build_parser().parse_args(COMMON + flags), physics=None)
    # the Gaussian model keeps accepting it, and --method sure has no equivariant branch
    losses.check_unsure_args(train.build_parser().parse_args(
        COMMON + ["--method", "proposed", "--no-ProposedLoss__stop_gradient", FLAG]))
    losses.check_unsure_args(train.build_parser().parse_args(
        COMMON + ["--method", "sure", "--no-ProposedLoss__stop_gradient"] + PG))
    with pytest.raises(ValueError, match="stop_gradient"):       # the constructor refuses the same combination by itself
        losses.ProposedLoss(blueprint={"ScalingTransform": {"kind": "padded", "antialias": False}}, sure_alternative=None,
                            noise_level=5, stop_gradient=False, sure_cropped_div=True, sure_averaged_cst=False,
                            sure_margin=2, alpha_tradeoff=1.0, transforms="Scaling_Transforms", physics=None, unsure=True,
                            unsure_noise_model="poisson_gaussian")


def test_the_existing_refusals_hold_for_the_model():
    import losses
    import train
    for method in ("proposed", "sure"):
        a = train.build_parser().parse_args(COMMON + ["--method", method] + PG)
        losses.check_unsure_args(a)                               # one GPU: accepted
        with pytest.raises(ValueError, match=FLAG):
            losses.check_unsure_args(a, world=2)
    for flags in (["--method", "proposed", "--ProposedLoss__sure_alternative", "r2r"], ["--method", "supervised"],
                  ["--method", "css"], ["--method", "noise2inverse"]):
        with pytest.raises(ValueError, match=FLAG):
            train.main(COMMON + flags + PG)


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
def test_get_loss_builds_the_eight_float_state_from_the_starting_guesses(method):
    import losses
    from losses.sure import SureGaussianLoss, SurePoissonGaussianLoss
    a = _namespace(method=method, sure_unknown_noise=True, unsure_noise_model="poisson_gaussian",
                   unsure_init_noise_level=15.0, unsure_init_gain=0.02, unsure_step_size=3e-4, unsure_momentum=0.5)
    term = losses.get_loss(a, physics=None).unsure_term()
    assert isinstance(term, SurePoissonGaussianLoss) and isinstance(term, SureGaussianLoss) and term.unsure
    assert (term.step_size, term.gain_step_size, term.momentum) == (3e-4, 3e-4, 0.5)     # the gain's step: the level's
    assert term.noise_state.dtype == torch.float32
    assert torch.equal(term.noise_state, torch.tensor([(15 / 255) ** 2, 0, 0, 0, 0.02, 0, 0, 0], dtype=torch.float32))
    assert [n for n, _ in term.named_buffers()] == ["noise_state"] and list(term.state_dict()) == ["noise_state"]
    assert abs(255 * term.estimated_sigma() - 15) < 1e-5 and term.estimated_gain() == float(L.f32(0.02))
    a.unsure_gain_step_size = 7e-5
    assert losses.get_loss(a, physics=None).unsure_term().gain_step_size == 7e-5
    # the state round-trips through state_dict in place; a Gaussian-length state does not load
    other = losses.get_loss(_namespace(method=method, sure_unknown_noise=True, unsure_noise_model="poisson_gaussian"),
                            physics=None).unsure_term()
    assert torch.equal(other.noise_state, torch.tensor([(5 / 255) ** 2, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float32))
    address = other.noise_state.data_ptr()
    other.load_state_dict(term.state_dict())
    assert torch.equal(other.noise_state, term.noise_state) and other.noise_state.data_ptr() == address
    gaussian = losses.get_loss(_namespace(method=method, sure_unknown_noise=True), physics=None).unsure_term()
    assert type(gaussian) is SureGaussianLoss and gaussian.noise_state.numel() == 4 and not hasattr(gaussian, "estimated_gain")
    with pytest.raises(RuntimeError):
        other.load_state_dict(gaussian.state_dict())


def test_entry_points_refuse_bad_arguments_on_the_host():
    """SEI_ERR_BAD_ARG before any HIP call (fake pointers: a refused call launches nothing and dereferences nothing)."""
    import _native
    lib = _native.lib()
    P_, Q = 4096, 4100
    ok = dict(y=P_, y1=P_, y2=P_, b=P_, planes=2, H=8, W=6, md=2, mm=2, tau=0.01, c_mse=0.1, inv_n_div=0.1, step_eta=1e-4,
              step_gamma=1e-4, mu=0.9, update=1, state=P_, out4=P_, g1=P_, g2=P_, work=P_, stream=None)
    assert len(ok) == len(_native.SIGNATURES["sei_sure_loss_unsure_pg"])
    bad = [dict(state=None), dict(state=Q), dict(state=P_ + 8), dict(mu=-0.1), dict(mu=1.0), dict(mu=float("nan")),
           dict(step_eta=float("inf")), dict(step_eta=float("nan")), dict(step_gamma=float("inf")),
           dict(step_gamma=float("-inf")), dict(step_gamma=float("nan")), dict(update=2), dict(update=-1),
           dict(md=3), dict(mm=3), dict(H=4), dict(tau=0.0), dict(planes=0), dict(y=None), dict(out4=None), dict(work=None)]
    for change in bad:
        assert lib.sei_sure_loss_unsure_pg(*dict(ok, **change).values()) == 10001, change
    assert lib.sei_axpy_hetero_dev(None, P_, P_, P_, 4, None) == 10001
    assert lib.sei_axpy_hetero_dev(P_, P_, None, P_, 4, None) == 10001
    assert lib.sei_axpy_hetero_dev(P_, P_, P_, P_, 0, None) == 10001
    for a, b, out in ((Q, P_, P_), (P_, Q, P_), (P_, P_, Q)):
        assert lib.sei_axpy_hetero_dev(a, b, P_, out, 8, None) == 10001
    assert lib.sei_axpy_hetero_dev(P_, P_, P_ + 2, P_, 8, None) == 10001


# ---------------------------------------------------------------------------------------------- get_physics
def _physics_args(**over):
    base = dict(task="deblurring", kernel="Gaussian_R2", sr_factor=None, noise_level=5, physics_v2=True,
                physics_true_adjoint=False)
    base.update(over)
    return argparse.Namespace(**base)


def test_get_physics_keeps_the_gaussian_model_without_a_gain():
    import physics
    from physics._base import GaussianNoise, PoissonGaussianNoise
    for args in (_physics_args(), _physics_args(noise_gain=0.0), _physics_args(noise_gain=0)):
        model = physics.get_physics(args, "cpu").noise_model
        assert type(model) is GaussianNoise and abs(model.sigma - 5 / 255) < 1e-12
    model = physics.get_physics(_physics_args(noise_gain=0.01), "cpu").noise_model
    assert type(model) is PoissonGaussianNoise and model.gain == 0.01 and abs(model.sigma - 5 / 255) < 1e-12
    with pytest.raises(ValueError, match="gain"):
        PoissonGaussianNoise(sigma=0.1, gain=-1.0)
