"""Cached bf16 copies of the weights, and the one place that decides whether a copy is still current.

A flattened model keeps a bf16 copy of its whole parameter bucket (`flat_shadow`; models/_flat.py), which the fused Adam
kernel rewrites every step. Three caches hang off the parameters: `shadow` (the (R, C) bf16 view of a 1x1-convolution
weight), `_transposed16_cached` (its transpose, for the fused MLP backward) and `split_x2` (the bf16x3 mode's head /
remainder planes). Their validity is a `ShadowState` per model plus one process-wide generation.
"""
import torch

import _native as N

_GLOBAL_GENERATION = 0      # bumped by weights_updated() without a model: every model's cached bf16 copies are suspect


class ShadowState:
    """Validity of a model's bf16 bucket (`flat_shadow`), tracked PER MODEL (`backbone._sei_plain_state`, shared with
    each of its parameters): `wgen` = this model's weight generation (bumped whenever its parameters change behind torch's
    version counters: its own optimizer kernel, its own load_state_dict), `gen` = the (global, own) generation pair the
    bf16 bucket was last written for, `version` = torch's version counter of each parameter when `shadow` last looked at
    it, `stale` = (start, stop) of the bucket whose float32 masters are OUT OF DATE on this rank (sharded optimizer step:
    only the bf16 copies of other ranks' shares were gathered) or None, `transposed` = every weight whose transposed bf16
    copy has been asked for, id(p) -> (p, w16)."""

    def __init__(self):
        self.wgen, self.gen, self.version, self.stale, self.transposed = 0, None, {}, None, {}

    def generation(self):
        return (_GLOBAL_GENERATION, self.wgen)

    def bump(self, plain_shadow_written=False):
        """The parameters changed; plain_shadow_written: and whoever changed them rewrote the bf16 bucket as well."""
        self.wgen += 1
        if plain_shadow_written:
            self.mark_current()

    def mark_current(self):
        self.gen = self.generation()

    def is_current(self):
        return self.gen == self.generation()

    def note_version(self, p):
        self.version[id(p)] = p._version

    def bucket_copy_current(self, p):
        """p's slice of the bf16 bucket is current: the bucket was written for this generation and torch has not changed p
        since `shadow` last looked at it."""
        return self.is_current() and self.version.get(id(p)) == p._version

    def set_stale(self, span):
        self.stale = None if span is None else (int(span[0]), int(span[1]))

    def stale_overlaps(self, p):
        """p's float32 values lie (or, without a known bucket offset, may lie) inside the stale range."""
        if self.stale is None:
            return False
        off = getattr(p, "_sei_bucket_offset", None)
        return off is None or (off < self.stale[1] and self.stale[0] < off + p.numel())

    @staticmethod
    def stale_error():
        return RuntimeError("the float32 weights of other ranks' shares are out of date on this rank (sharded optimizer "
                            "step: only their bf16 copies were all-gathered) and something asked for bf16 copies to be "
                            "rebuilt from them; call optimizer.consolidate() on every rank before changing or re-reading "
                            "the weights")


_new_plain_state = ShadowState


def _cache_key(p, ptr, capture_sensitive):
    """The key a cached bf16 copy of parameter p is valid for: (generation, torch's version counter, address of what it
    was built from). Capture-sensitive caches -- `split_x2` and the transposed copies -- add whether the stream is
    capturing: they are rebuilt once inside a capture, so that every replay rebuilds them from the weights of ITS step.
    `shadow` is NOT capture-sensitive: it is a view of the bf16 bucket, which the optimizer kernel itself keeps current."""
    state = getattr(p, "_sei_plain_state", None)
    key = (state.generation() if state is not None else (_GLOBAL_GENERATION, 0), p._version, ptr)
    return key + (torch.cuda.is_current_stream_capturing(),) if capture_sensitive else key


def weights_updated(backbone=None, plain_shadow_written=False):
    """Parameters changed outside torch's version counters. With a `backbone` only THAT model's cached bf16 copies are
    invalidated (another model's optimizer step or load_state_dict must not make this one recast its weights: under a
    sharded optimizer step the float32 masters of other ranks' shares are stale and a recast would overwrite good bf16
    weights with old values); without one, every model's. `plain_shadow_written`: the optimizer kernel also refreshed
    `backbone.flat_shadow` (the bf16 copy of every parameter), so that copy is current for the new generation."""
    global _GLOBAL_GENERATION
    if backbone is None:
        _GLOBAL_GENERATION += 1
        return
    backbone._sei_plain_state.bump(plain_shadow_written)


def plain_shadow_is_current(backbone):
    return backbone._sei_plain_state.is_current()


def set_stale_masters(backbone, span):
    """optim.FlatAdam (sharded step): float32 parameters inside bucket range `span` are stale on this rank until
    `consolidate()`; None clears it. While set, nothing may rebuild bf16 copies of that range from the masters."""
    backbone._sei_plain_state.set_stale(span)


def refresh_plain_shadow(backbone):
    """Cast the whole flat parameter bucket to its bf16 copy (what the fused Adam does as a side output)."""
    if getattr(backbone, "flat_shadow", None) is None:
        return
    state = backbone._sei_plain_state
    if state.stale is not None:
        raise state.stale_error()
    N.call("sei_cast_bf16", backbone.flat_params.data_ptr(), backbone.flat_shadow.data_ptr(),
           backbone.flat_params.numel())
    state.mark_current()


def shadow(p):
    """bf16 copy w16 (R,C) of a 1x1-conv weight p (R,C,1,1): a view of the owning model's flat bf16 bucket,
    which the fused Adam kernel rewrites every step; cast here only when that copy is not current.
    (No transposed copy exists: the data-gradient GEMM reads w16 reduction-major.)"""
    state = getattr(p, "_sei_plain_state", None)
    key = _cache_key(p, p.data_ptr(), False)
    st = getattr(p, "_sei_shadow", None)
    if st is None or st[0] != key:
        R, C = p.shape[0], p.shape[1]
        flat16 = getattr(p, "_sei_shadow_view", None)
        if st is not None and st[1].device == p.device:
            w16 = st[1]
        else:
            w16 = flat16.view(R, C) if flat16 is not None else torch.empty((R, C), dtype=torch.bfloat16, device=p.device)
        if not (flat16 is not None and state is not None and state.bucket_copy_current(p)):
            if state is not None and state.stale_overlaps(p):
                raise state.stale_error()
            N.call("sei_cast_bf16", p.data_ptr(), w16.data_ptr(), p.numel())
        if state is not None:
            state.note_version(p)
        st = (key, w16)
        p._sei_shadow = st
    return st[1]


def _transposed16_cached(p, w16):
    """_transposed16 of a weight's bf16 copy, rebuilt only when the copy changed (one optimizer step = one rebuild, not
    one per backward function: the step's two model calls share it). Every weight that has ever asked is remembered per
    model; when one of them is stale, ALL stale ones are rebuilt by one sei_transpose_bf16_many launch (the 8 matrices of the
    two fused levels: one launch per step instead of 8 of ~9 us each)."""
    state = getattr(p, "_sei_plain_state", None)
    key = _cache_key(p, w16.data_ptr(), True)
    hit = getattr(p, "_sei_shadow_t", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    group = state.transposed if state is not None else {}
    group[id(p)] = (p, w16)
    stale = []
    for q, q16 in group.values():
        qkey = _cache_key(q, q16.data_ptr(), True)
        qhit = getattr(q, "_sei_shadow_t", None)
        if qhit is None or qhit[0] != qkey:
            # another weight rides along only while its bf16 copy in the bucket is known to be current; anything else is
            # rebuilt when its layer asks, after `shadow` has had its look
            if q is p or (state is not None and state.bucket_copy_current(q)):
                stale.append((q, q16, qkey))
    if len(stale) == 1 or not p.is_cuda:
        hit = (key, _transposed16(w16))
        p._sei_shadow_t = hit
        return hit[1]
    for k in range(0, len(stale), N.TRANSPOSE_MAX_JOBS):
        part = stale[k:k + N.TRANSPOSE_MAX_JOBS]
        outs = [torch.empty((q16.shape[1], q16.shape[0]), dtype=torch.bfloat16, device=q16.device) for _, q16, _ in part]
        jobs = (N.TransposeJob * len(part))(*[N.TransposeJob(q16.data_ptr(), o.data_ptr(), q16.shape[0], q16.shape[1])
                                             for (_, q16, _), o in zip(part, outs)])
        N.call("sei_transpose_bf16_many", jobs, len(part))
        for (q, _, qkey), o in zip(part, outs):
            q._sei_shadow_t = (qkey, o)
    return p._sei_shadow_t[1]


def _transposed16(w16):
    """(R, C) bf16 -> (C, R) bf16 copy (data movement; the fused MLP backward reads both weights transposed)."""
    R, C = w16.shape
    wt = torch.empty((C, R), dtype=torch.bfloat16, device=w16.device)
    N.call("sei_cast_transpose_bf16", w16.data_ptr(), 1, None, wt.data_ptr(), R, C, R, None)
    return wt


def split_x2(t):
    """(2, *t.shape) bf16: head and remainder planes of a float32 tensor. A parameter's planes are cached until its
    values change (this model's optimizer kernel / load_state_dict, torch's version counter: `_cache_key`) -- and rebuilt
    once inside a capture, so that every replay splits the weights of ITS step."""
    def fresh():
        planes = torch.empty((2,) + tuple(t.shape), dtype=torch.bfloat16, device=t.device)
        N.call("sei_split_bf16x2", t.data_ptr(), planes.data_ptr(), t.numel())
        return planes
    if not isinstance(t, torch.nn.Parameter):
        return fresh()
    key = _cache_key(t, t.data_ptr(), True)
    hit = getattr(t, "_sei_split", None)
    if hit is None or hit[0] != key:
        hit = (key, fresh())
        t._sei_split = hit
    return hit[1]
