"""float64 model of one torch.optim.Adam step (single-tensor form, amsgrad=False, coupled weight decay), the inputs and
the stage-wise rounding bounds that the Adam kernels are held to (tests/test_adam_ref.py anchors the model to
torch.optim.Adam itself; tests/test_adam_gpu.py compares every kernel that inlines sei_adam_element with it).

Plain numpy: nothing of the library under test is imported here. The hyper-parameters are rounded to float32 first (the
C ABI takes `float`), then used as float64; 1.f - beta is exact in float32 for beta >= 0.5, which every set below
respects, so the model and a kernel see the same 1 - beta.

Why the bounds are stage-wise: comparing the final p' with a float64 run from the OLD state amplifies the cancellation
in g + wd p and in g2 - m by 1 / denom (a correct float32 emulation sits 1800 u off such a model). So every stage is
compared with float64 of that stage's own inputs. u = 2^-24, S = |grad_scale g| + |wd p|, (m_k, v_k, p_k) a kernel's
results, per element, no max-norm:
    m':  |m_k - m'| <= 4 u (|m| + S)                    three roundings and the weight-decay FMA
    v':  |v_k - v'| <= 8 u (b2 v + (1 - b2) S^2)        g2's relative error twice through the square, three roundings
    p':  |p_k - (p - delta_k)| <= u |p| + 8 u |delta_k|  delta_k = the float64 update formula evaluated from (m_k, v_k):
         sqrt, two multiplies, add, divide, the two rounded scalars and the final subtraction
A float32 emulation without FMA contraction (emulate32 below) reaches 1.7 u, 5.2 u and 4.5 u (|p| + |delta|) of these
scales over the five sets and both gradient scales (tests/test_adam_ref.py prints them).
"""
import collections
import functools

import numpy as np

U = 2.0 ** -24
BOUND_M, BOUND_V, BOUND_DELTA = 4.0, 8.0, 8.0

Hyper = collections.namedtuple("Hyper", "lr beta1 beta2 eps weight_decay step")
# elements on both sides of sqrt(v) ~ eps and of |g| ~ wd |p|; steps 1 (zero moments) to 10^5 (bias corrections ~ 1)
HYPER_SETS = (Hyper(1e-3, 0.9, 0.999, 1e-8, 0.0, 1),
              Hyper(2e-4, 0.9, 0.99, 1e-8, 0.01, 5),
              Hyper(1e-4, 0.5, 0.9, 1e-3, 0.1, 2),
              Hyper(1e-4, 0.9, 0.999, 1e-8, 0.0, 100000),
              Hyper(3e-4, 0.95, 0.9999, 1e-12, 1e-2, 1000))
N_MAIN = 100003
MIN_INFORMATIVE = 0.85      # share of elements whose update exceeds the rounding of p: below, the p check says nothing


def f32(x):
    """The value a `float` argument of the C ABI carries, as a Python float."""
    return float(np.float32(x))


def rounded(hyper):
    return Hyper(*(f32(x) for x in hyper[:5]), int(hyper.step))


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def delta64(m1, v1, hyper):
    """torch's update lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps) from the NEW moments, in float64."""
    h = rounded(hyper)
    bc1 = 1.0 - h.beta1 ** h.step
    bc2 = 1.0 - h.beta2 ** h.step
    return (h.lr / bc1) * (_f64(m1) / (np.sqrt(_f64(v1)) / np.sqrt(bc2) + h.eps))


def adam_step64(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    """(p', m', v', delta) of torch's single-tensor Adam step number `step` in float64."""
    h = rounded(Hyper(lr, beta1, beta2, eps, weight_decay, step))
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    g2 = f32(grad_scale) * g + h.weight_decay * p
    m1 = m + (g2 - m) * (1.0 - h.beta1)
    v1 = h.beta2 * v + (1.0 - h.beta2) * g2 * g2
    delta = delta64(m1, v1, h)
    return p - delta, m1, v1, delta


def scales(p, g, m, v, hyper, grad_scale=1.0):
    """(scale of the m' bound, scale of the v' bound): |m| + S and b2 v + (1 - b2) S^2."""
    h = rounded(hyper)
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    s = np.abs(f32(grad_scale) * g) + np.abs(h.weight_decay * p)
    return np.abs(m) + s, h.beta2 * v + (1.0 - h.beta2) * s * s


Worst = collections.namedtuple("Worst", "m v p")


def _worst(err, scale):
    """max err / scale over the elements with a scale; an element without one must be exact."""
    assert not np.any((scale == 0) & (err != 0)), "an element whose scale is zero is not exact"
    return float(np.max(np.divide(err, scale, out=np.zeros_like(err), where=scale > 0), initial=0.0))


def stage_errors(p, g, m, v, pk, mk, vk, hyper, grad_scale=1.0):
    """Worst(m, v, p): the largest error of each stage over the elements, m and v in units of u x their scale (bounds
    BOUND_M, BOUND_V), p in units of u (|p| + |delta_k|) -- the figure that is recorded; check_stages asserts the bounds."""
    _, m1, v1, _ = adam_step64(p, g, m, v, grad_scale=grad_scale, **hyper._asdict())
    sm, sv = scales(p, g, m, v, hyper, grad_scale)
    mk, vk, pk, p = _f64(mk), _f64(vk), _f64(pk), _f64(p)
    dk = delta64(mk, vk, hyper)
    ep = np.abs(pk - (p - dk))
    return (Worst(_worst(np.abs(mk - m1), U * sm), _worst(np.abs(vk - v1), U * sv), _worst(ep, U * (np.abs(p) + np.abs(dk)))),
            ep, U * np.abs(p) + BOUND_DELTA * U * np.abs(dk))


def check_stages(p, g, m, v, pk, mk, vk, hyper, grad_scale=1.0, what=""):
    """Assert the three stage-wise bounds for every element; returns Worst for the record. All arguments finite."""
    for name, a in (("p", pk), ("exp_avg", mk), ("exp_avg_sq", vk)):
        assert np.all(np.isfinite(_f64(a))), f"{what}: {name} is not finite"
    worst, ep, bound_p = stage_errors(p, g, m, v, pk, mk, vk, hyper, grad_scale)
    assert worst.m <= BOUND_M, f"{what}: exp_avg off by {worst.m:.3g} u (|m| + S), bound {BOUND_M}"
    assert worst.v <= BOUND_V, f"{what}: exp_avg_sq off by {worst.v:.3g} u (b2 v + (1 - b2) S^2), bound {BOUND_V}"
    over = ep > bound_p
    assert not over.any(), (f"{what}: p off its own moments' update at {int(over.sum())} elements, worst "
                            f"{worst.p:.3g} u (|p| + |delta|); bound u |p| + {BOUND_DELTA} u |delta|")
    return worst


def informative_fraction(p, g, m, v, hyper, grad_scale=1.0):
    """Share of the elements with |delta| > u |p| in the float64 model: the ones whose p' tells the update."""
    _, _, _, delta = adam_step64(p, g, m, v, grad_scale=grad_scale, **hyper._asdict())
    return float(np.mean(np.abs(delta) > U * np.abs(_f64(p))))


def _log_uniform(rng, n, lo, hi, signed):
    mag = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    return (mag * rng.choice((-1.0, 1.0), n) if signed else mag).astype(np.float32)


@functools.lru_cache(maxsize=None)
def state(n, first_step=False, seed=0):
    """(p, g, m, v) float32, read-only, built once per (n, first_step, seed): log-uniform magnitudes with random sign,
    p in [1e-6, 10], g and m in [1e-12, 1e3], v in [1e-24, 1e6] (g^2 stays above the float32 denormals; gradients under
    3e-18, where float32 v underflows and float64 does not, are left to the special-value tables); m = v = 0 at step 1."""
    rng = np.random.default_rng(1000 + seed)
    p = _log_uniform(rng, n, 1e-6, 10.0, True)
    g = _log_uniform(rng, n, 1e-12, 1e3, True)
    m = _log_uniform(rng, n, 1e-12, 1e3, True)
    v = _log_uniform(rng, n, 1e-24, 1e6, False)
    if first_step:
        m, v = np.zeros_like(m), np.zeros_like(v)
    for a in (p, g, m, v):
        a.setflags(write=False)
    return p, g, m, v


def case(hyper, n=N_MAIN, seed=0):
    """The inputs of one hyper-parameter set at n elements; at the main size the p check must not be vacuous."""
    arrays = state(n, first_step=hyper.step == 1, seed=seed)
    if n >= N_MAIN:
        share = informative_fraction(*arrays, hyper)
        assert share >= MIN_INFORMATIVE, f"{hyper}: only {share:.3f} of the updates exceed the rounding of p"
    return arrays


def emulate32(p, g, m, v, hyper, grad_scale=1.0):
    """The update in float32, operation by operation, without FMA contraction (the scalars lr / bc1 and 1 / sqrt(bc2)
    from float64 arithmetic, rounded once): what a correct float32 implementation computes, up to contraction."""
    h = rounded(hyper)
    f = np.float32
    step_size = f(h.lr / (1.0 - h.beta1 ** h.step))
    inv_bc2_sqrt = f(1.0 / np.sqrt(1.0 - h.beta2 ** h.step))
    p, m, v = (np.asarray(a, dtype=f) for a in (p, m, v))
    g2 = np.asarray(g, dtype=f) * f(grad_scale)
    if h.weight_decay != 0.0:
        g2 = f(h.weight_decay) * p + g2
    m1 = m + (g2 - m) * (f(1) - f(h.beta1))
    v1 = f(h.beta2) * v + (f(1) - f(h.beta2)) * g2 * g2
    denom = np.sqrt(v1) * inv_bc2_sqrt + f(h.eps)
    return p - step_size * (m1 / denom), m1, v1
