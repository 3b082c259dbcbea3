"""Restatement of deepinv 0.2's sampling.DiffPIR (tables, noise schedule, forward) and of the expressions of the fused
DiffPIR kernels, in any dtype: the pinned truth of tests/test_diffpir_baseline.py and tests/test_diffpir_baseline_gpu.py.
Written from deepinv's published DiffPIR.get_alpha_beta / get_noise_schedule / find_nearest / forward with torch tensors,
as deepinv holds them, independently of models/diffpir.py (which uses numpy). Not collected."""
import math

import numpy as np
import torch

from drunet_ref import cg_ref, forward_ref

T = 1000


def tables_ref():
    """float32 torch tensors of length 1000: (sa, s1m, red, srec) = sqrt(ac), sqrt(1 - ac), their ratio, sqrt(1 / ac)."""
    betas = torch.from_numpy(np.linspace(0.1 / 1000, 20 / 1000, T, dtype=np.float32))
    ac = torch.cumprod(1.0 - betas, dim=0)
    sa, s1m = torch.sqrt(ac), torch.sqrt(1.0 - ac)
    return sa, s1m, torch.div(s1m, sa), torch.sqrt(1.0 / ac)


def schedule_ref(sigma, lambda_, max_iter):
    """(rhos, sigmas, seq): the element-by-element loop of get_noise_schedule."""
    sa, s1m, red, _ = tables_ref()
    sigmas, rhos = [], []
    for i in range(T):
        sigmas.append(red[T - 1 - i])
        sigma_k = s1m[i] / sa[i]
        rhos.append(lambda_ * (sigma ** 2) / (sigma_k ** 2))
    seq = [int(s) for s in list(np.sqrt(np.linspace(0, T ** 2, max_iter)))]
    seq[-1] = seq[-1] - 1
    return torch.tensor(rhos), torch.tensor(sigmas), seq


def nearest_ref(value):
    red = tables_ref()[2]
    return int(np.abs(np.asarray(red) - np.asarray(value)).argmin())


# ---- the expressions of the fused kernels, literally ----

def prologue_ref(o, Aty, inv_gamma):
    """b of sei_cg_init with the DiffPIR prologue."""
    return Aty + ((2 * o - 1).clamp(-1, 1) / 2 + 0.5) * inv_gamma


def sample_ref(u, x, nz, sa_t, s1m_t, sa_n, s1m_n, zeta, at_n):
    """(next x, next denoiser input, max-abs of every operand per element) of sei_diffpir_sample. Scalars are floats; the
    arithmetic runs in the dtype of the tensors."""
    c_eps, c_nz, den = math.sqrt(1 - zeta), math.sqrt(zeta), 2 * math.sqrt(at_n)
    x0 = 2 * u - 1
    a = sa_t * x0
    eps = (x - a) / s1m_t
    inner = c_eps * eps + c_nz * nz
    xn = sa_n * x0 + s1m_n * inner
    xin = xn / den + 0.5
    big = torch.stack([t.abs().double() for t in (2 * u, x0, x, a, x - a, eps, c_eps * eps, c_nz * nz, inner,
                                                  s1m_n * inner, sa_n * x0, xn)]).amax(0)
    return xn, xin, big, torch.maximum(big / den, xin.abs().double()).clamp_min(0.5)


def cg_history_ref(op, b, max_iter):
    """cg_ref with tol = 0, also returning the residual norm after every iteration."""
    x = torch.zeros_like(b)
    r = b.clone()
    p = r
    rs = (r * r).sum()
    norms = []
    for _ in range(max_iter):
        Ap = op(p)
        alpha = rs / (p * Ap).sum()
        x = x + alpha * p
        r = r - alpha * Ap
        rs_new = (r * r).sum()
        norms.append(math.sqrt(float(rs_new)))
        p = r + (rs_new / rs) * p
        rs = rs_new
    return x, norms


def diffpir_ref(y, A, At, sd, sigma, dtype, draws, max_iter=100, zeta=0.1, lambda_=7.0, cg_max_iter=50, cg_tol=1e-3,
                round_bf16=False):
    """DiffPIR.forward in `dtype` with the float32 tables and schedule deepinv holds; A / At are callables in that dtype,
    `draws[i]` the standard normal tensors (0: the initial noise, k + 1: sampling step k). Returns (x, proxes run)."""
    sa, s1m, red, srec = tables_ref()
    rhos, sigmas, seq = schedule_ref(sigma, lambda_, max_iter)
    y = y.to(dtype)
    Aty = At(y)
    x = 2 * Aty - 1
    proxes = 0
    x0 = None
    for i in range(len(seq)):
        cs = float(sigmas[seq[i]])
        t = nearest_ref(cs)
        at = 1.0 / float(srec[t]) ** 2
        if i == 0:
            x = (x + cs * draws[0].to(dtype)) / float(srec[-1])
        out = forward_ref(sd, x / (2 * math.sqrt(at)) + 0.5, cs / 2, dtype, round_bf16)
        x0 = (2 * out - 1).clamp(-1, 1)
        if not seq[i] == seq[-1]:
            gamma = 1.0 / (2.0 * float(rhos[t]))
            u = cg_ref(lambda v: At(A(v)) + v / gamma, Aty + (x0 / 2 + 0.5) / gamma, cg_max_iter, cg_tol)
            proxes += 1
            x0 = u * 2 - 1
            tn = nearest_ref(float(sigmas[seq[i + 1]]))
            eps = (x - float(sa[t]) * x0) / float(s1m[t])
            x = float(sa[tn]) * x0 + float(s1m[tn]) * (math.sqrt(1 - zeta) * eps + math.sqrt(zeta) * draws[i + 1].to(dtype))
    return x0 / 2 + 0.5, proxes
