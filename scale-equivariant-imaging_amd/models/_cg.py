"""Conjugate gradients with the scalars on the device: the host side of the sei_cg_* kernels (csrc/diffpir_kernels.hip).

FusedCG(n, device) owns the work buffers of one solve of (A^T A + I / gamma) u = A^T y + u0 / gamma from zero over n floats
and the SeiCgState block that holds rs, pAp, rs_new, the stopping flag and the iteration count. An iteration is the
caller's `op` (the physics' own A / A_adjoint kernels) and three entry points, each followed by its one-workgroup fold;
no value of the solve is read by the host inside it. The recurrences are deepinv v0.2.0's conjugate_gradient, the ones
models/pnp.py runs as torch expressions with one host read per iteration.

The stopping test runs on the device: once sqrt(rs_new) < tol the kernels of every later iteration return without
writing, so the host may run ahead. It copies the flag back once every `poll` iterations and stops launching when it is
set; the result is the same bits for every `poll`.
"""
import torch

import _native as N


class FusedCG:
    def __init__(self, n, device):
        n = int(n)
        if n < 1:
            raise ValueError("FusedCG: n >= 1")
        self.n = n
        f32 = dict(dtype=torch.float32, device=device)
        self.x, self.r, self.p, self.Ap, self.AtAp = (torch.empty(n, **f32) for _ in range(5))
        self.part = torch.empty(int(N.lib().sei_cg_partials(n)), **f32)
        self.state = torch.zeros(N.CG_STATE_WORDS, dtype=torch.int32, device=device)
        self.iterations = 0
        self.launched = 0            # iterations enqueued by the last solve (>= iterations: the host runs ahead of the flag)

    def _flag(self):
        done, count = self.state[N.CG_DONE:N.CG_ITERATIONS + 1].tolist()      # one copy, one wait
        return bool(done), int(count)

    def _operand(self, t, name):
        N.check_tensor(t, name)
        if t.numel() != self.n:
            raise ValueError(f"FusedCG: {name} has {t.numel()} elements, the solver was built for {self.n}")
        return t if N.aligned(t) else t.clone()

    def solve(self, op, u0, Aty, gamma, max_iter, tol, poll=5, prologue=False):
        """x of deepinv's conjugate_gradient(v -> A^T A v + v / gamma, Aty + u0 / gamma, max_iter, tol), in self.x (n
        floats, overwritten by the next solve). `op(p, out)` returns A^T A p for the flat n-element `p` as a contiguous
        float32 tensor of n elements: `out`, a buffer of the solver's, where the operator can write into one, else a
        tensor of its own (the physics' kernels allocate their results). With `prologue`
        u0 is the denoiser output o and clamp(2 o - 1, -1, 1) / 2 + 0.5 takes its place. `iterations` is the device's count
        of updates made: max_iter, or the iteration whose residual fell below tol."""
        gamma, tol, max_iter, poll = float(gamma), float(tol), int(max_iter), int(poll)
        if not gamma > 0 or gamma == float("inf"):
            raise ValueError(f"FusedCG: gamma must be positive and finite, got {gamma}")
        if poll < 1 or max_iter < 0:
            raise ValueError("FusedCG: poll >= 1 and max_iter >= 0")
        u0, Aty = self._operand(u0, "u0"), self._operand(Aty, "Aty")
        inv_gamma = 1.0 / gamma
        x, r, p, Ap, part, state = (t.data_ptr() for t in (self.x, self.r, self.p, self.Ap, self.part, self.state))
        n = self.n
        N.call("sei_cg_init", u0.data_ptr(), Aty.data_ptr(), inv_gamma, int(bool(prologue)), x, r, p, part, state, n)
        done, count, it = False, 0, 0
        while it < max_iter:
            AtAp = self._operand(op(self.p, self.AtAp), "op's result")
            N.call("sei_cg_apply", p, AtAp.data_ptr(), inv_gamma, Ap, part, state, n)
            N.call("sei_cg_update", x, r, p, Ap, tol, part, state, n)
            N.call("sei_cg_direction", p, r, state, n)
            it += 1
            if (tol > 0 and it % poll == 0) or it == max_iter:          # (tol = 0 never stops early: nothing to poll for)
                done, count = self._flag()
                if done:
                    break
        self.launched, self.iterations = it, count
        return self.x
