"""tests/adam_ref.py against torch.optim.Adam itself, on the CPU: the float64 model that tests/test_adam_gpu.py holds the
HIP kernels to is anchored to torch before anything is compared with it, and the stage-wise bounds are shown to pass a
correct float32 implementation and to refuse four wrong ones."""
import numpy as np
import pytest
import torch

import adam_ref as R


@pytest.mark.parametrize("hyper", R.HYPER_SETS, ids=lambda h: f"step{h.step}")
def test_model_is_torch_adam_in_float64(hyper):
    """Four steps with fresh gradients from the set's own state: p, exp_avg and exp_avg_sq of adam_step64 equal
    torch.optim.Adam(foreach=False) on float64 tensors, given the same float32-rounded hyper-parameters as Python floats,
    to 1e-12 relative per element."""
    n = 4096
    h = R.rounded(hyper)
    p0, _, m0, v0 = R.state(n, first_step=hyper.step == 1)
    param = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
    opt = torch.optim.Adam([param], lr=h.lr, betas=(h.beta1, h.beta2), eps=h.eps, weight_decay=h.weight_decay,
                           foreach=False)
    if hyper.step > 1:                                  # torch's own state, as a checkpoint of step - 1 would leave it
        opt.state[param] = {"step": torch.tensor(float(hyper.step - 1)),
                            "exp_avg": torch.from_numpy(m0.astype(np.float64)),
                            "exp_avg_sq": torch.from_numpy(v0.astype(np.float64))}
    p, m, v = (a.astype(np.float64) for a in (p0, m0, v0))
    for k in range(4):
        g = R.state(n, seed=10 + k)[1].astype(np.float64)
        param.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v, _ = R.adam_step64(p, g, m, v, **h._replace(step=hyper.step + k)._asdict())
        st = opt.state[param]
        assert float(st["step"]) == hyper.step + k
        for mine, theirs in ((p, param.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            np.testing.assert_allclose(mine, theirs.numpy(), rtol=1e-12, atol=0)


@pytest.mark.parametrize("hyper", R.HYPER_SETS, ids=lambda h: f"step{h.step}")
def test_inputs_keep_the_parameter_check_informative(hyper):
    """At the main size at least 85 % of the updates exceed the rounding of p in the float64 model (adam_ref.case
    asserts it); the draws are read-only and the same on every call."""
    arrays = R.case(hyper)
    assert all(a.dtype == np.float32 and not a.flags.writeable and a.shape == (R.N_MAIN,) for a in arrays)
    assert all(a is b for a, b in zip(arrays, R.case(hyper)))
    p, g, m, v = arrays
    assert np.all(v >= 0) and float(np.abs(g).min()) >= 1e-12 * (1 - 1e-6)
    assert (hyper.step == 1) == (not m.any() and not v.any())


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("hyper", R.HYPER_SETS, ids=lambda h: f"step{h.step}")
def test_bounds_pass_a_correct_float32_update_and_refuse_wrong_ones(hyper, grad_scale):
    """emulate32 (float32, no contraction) stays inside the three bounds; an update with eps inside the square root,
    decoupled weight decay, the bias corrections of step t - 1 or the gradient scale applied after the weight decay
    leaves them wherever the set can tell the difference."""
    p, g, m, v = R.case(hyper)
    pk, mk, vk = R.emulate32(p, g, m, v, hyper, grad_scale)
    worst = R.check_stages(p, g, m, v, pk, mk, vk, hyper, grad_scale, what="float32 emulation")
    print(f"float32 emulation, step {hyper.step}, grad_scale {grad_scale}: {worst}")

    h = R.rounded(hyper)
    f = np.float32
    step_size = f(h.lr / (1.0 - h.beta1 ** h.step))
    inv = f(1.0 / np.sqrt(1.0 - h.beta2 ** h.step))

    def refused(pk, mk, vk):
        try:
            R.check_stages(p, g, m, v, pk, mk, vk, hyper, grad_scale)
        except AssertionError:
            return True
        return False

    # eps inside the square root
    assert refused(p - step_size * (mk / (np.sqrt(vk * inv * inv + f(h.eps))).astype(f)), mk, vk)
    # the bias corrections of step t - 1 (step 1 has no predecessor: its successor's), where float32 can tell them apart
    other = h._replace(step=h.step - 1 if h.step > 1 else 2)
    ratio1 = (1.0 - h.beta1 ** other.step) / (1.0 - h.beta1 ** h.step)
    ratio2 = np.sqrt((1.0 - h.beta2 ** other.step) / (1.0 - h.beta2 ** h.step))
    if max(abs(ratio1 - 1.0), abs(ratio2 - 1.0)) > 32 * R.U:
        assert refused(*R.emulate32(p, g, m, v, other, grad_scale))
    if h.weight_decay:
        # decoupled (AdamW) decay: the moments see the bare gradient
        pw, mw, vw = R.emulate32(p * f(1.0 - h.lr * h.weight_decay), g, m, v, h._replace(weight_decay=0.0), grad_scale)
        assert refused(pw, mw, vw)
    if h.weight_decay and grad_scale != 1.0:
        # (g + wd p) * grad_scale
        g_late = (f(h.weight_decay) * p + g) * f(grad_scale)
        assert refused(*R.emulate32(p, g_late, m, v, h._replace(weight_decay=0.0), 1.0))
