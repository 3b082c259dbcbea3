"""The weight-gradient scheduler: when, and as which launch, the weight gradient of a 1x1 convolution (or a linear
layer of a Swin block) is issued. The layer functions (models/_ops.py, models/_swin_ops16.py) hand their operand pairs
to `weight_grad16` / `weight_grad16_group` and their partial sums to `defer_fold`; everything else here is bookkeeping
per backbone (`WeightGradState`), reached through thin module-level functions: ONE record per gradient (`GradRecord`,
whose docstring says which field lives how long), the pairs parked for the step's other model call, the queued streamed
jobs and the deferred folds.
"""
import collections
import os
import weakref

import torch

import _native as N
from . import _gemm
from ._gemm import EPI_ACCUM, EPI_NONE, _gemm_call, gemm_mixed, gemm_nt16

# The token-streaming kernels of token_gemm.hip (Swin blocks) against the tiled GEMMs they replace: on unless
# SEI_SWIN_TILED=1 (tests flip the flag to run the same step on both paths; shapes the streaming kernels do not take --
# token counts that are not multiples of 64 -- use the tiled ones anyway).
TOKEN_STREAMING = os.environ.get("SEI_SWIN_TILED") != "1"

# Streamed weight gradients of the shallow levels (csrc/dw_stream.hip): the accumulating weight gradients whose shapes
# sei_dwstream_bf16_eligible takes -- conv2 / conv3 of the C = 32 and C = 128 blocks, the 1x1 convolutions between the
# 32-, 128- and 512-channel levels -- are not launched one by one on the tiled GEMM (a 128 x 128 output tile under up to
# 256 K-splits) but collected, operands kept alive, and issued as ONE job table when the backward pass ends (the engine
# callback that flushes parked pairs and deferred folds), or at once outside a backward pass. SEI_NO_DWSTREAM=1: the GEMMs.
DWSTREAM = os.environ.get("SEI_NO_DWSTREAM") != "1"

# Deferred folds. The reducing kernels of a backward pass (LayerNorm parameter gradients, depthwise weight gradients,
# the LayerNorm epilogue of SwinIR's data-gradient GEMMs) leave per-workgroup partial sums; instead of one ~5-us fold
# launch behind each of them (52 per U-Net step, ~146 per SwinIR step) the partial sums are kept alive and ONE
# sei_fold_many launch per <= 40 destinations adds them up when the backward pass ends (the engine callback that also
# flushes parked weight gradients). Both ways run one device routine (fold_entries in csrc/reduce_kernels.hip, where the
# order of the additions is stated; oracle/fold_order.py is its model), launches of one destination one after the other:
# bit-identical gradients. Outside a backward pass (kernel-level tests calling the helpers directly) nothing is
# deferred. SEI_NO_DEFERRED_FOLDS=1 restores the fold per launch.
DEFERRED_FOLDS = os.environ.get("SEI_NO_DEFERRED_FOLDS") != "1"

# The two epilogue sinks: the step's complete gradient is consumed by the epilogue of the GEMM that produces it. kind ->
# (entry point, what a refusal calls it); the views registered with a kind are that entry point's arguments after the operands.
SINK_ADAM, SINK_BF16 = "adam", "direct16"
_SINKS = {SINK_ADAM: ("sei_gemm_bf16nt_dw2_adam", "fused optimizer step"),
          SINK_BF16: ("sei_gemm_bf16nt_dw2_bf16out", "bf16 gradients written into the exchange buffer")}

# Grouped fused-Adam launches. A SINK_ADAM weight gradient of whole 128 x 256 tiles that alone runs a single round of
# workgroups (N.adam_gemm_groupable: the rule lives in csrc/gemm_bf16nt.hip beside adam_wide_auto) is not launched where it
# arrives but queued, operands kept alive, and the queue goes out as ONE sei_gemm_bf16nt_dw2_adam_group launch per <= 8
# jobs when the backward pass ends: the main loops of one job then run under the parameter streams of another, where a
# launch of its own runs all its loops and then all its epilogues. Deferring is safe because
#   * a weight's bf16 copy is read in the backward pass only by its own layer's data-gradient GEMMs, and every layer
#     function issues those BEFORE it hands in the weight gradient (models/_ops.py, ConvBlockFn16.backward);
#   * nothing between the arrival and the end of the backward pass reads the parameter, its moments or its copy: the
#     optimizer's own pass, the shadow refresh and the next forward all follow the engine callback;
#   * SINK_ADAM is registered only without a reducer (graphs.GraphedLossStep._plan_sinks), and while a milestone is set
#     (early release) nothing is queued: the event never waits for a deferred launch.
# Outside a backward pass nothing is deferred. SEI_NO_ADAM_GROUP=1: every launch where it arrives, as before.
ADAM_GROUP = os.environ.get("SEI_NO_ADAM_GROUP") != "1"

_Queued = collections.namedtuple("_Queued", "job operands grad flops")     # one entry of WeightGradState.dwjobs
_QueuedAdam = collections.namedtuple("_QueuedAdam", "job operands hyper flops args")   # one of WeightGradState.adamjobs


def _segments(pairs):
    """(g1, x1, g2, x2, K1, K2) of the one or two (gy16, x16) row segments of a launch; a single one stands twice, K2 = 0."""
    (g1, x1), (g2, x2) = pairs[0], pairs[-1]
    return g1, x1, g2, x2, g1.shape[0], (g2.shape[0] if len(pairs) == 2 else 0)


def colsum16_into(acc, x16):
    """acc[n] += sum_m x16[m, n]: a bias gradient from the bf16 gradient of the layer's output."""
    M, Nn = x16.shape
    N.call("sei_colsum_bf16", x16.data_ptr(), acc.data_ptr(), M, Nn)


def _dwstream_ok(grad2d, pairs):
    """The streamed launch serves this weight gradient (shapes, layouts, pixel counts)."""
    if not DWSTREAM or not grad2d.is_cuda or grad2d.dim() != 2 or grad2d.dtype != torch.float32 or len(pairs) > 2 \
            or grad2d.stride(1) != 1:
        return False
    Np, Kp = grad2d.shape
    for gy, x in pairs:
        if not (gy.dtype == x.dtype == torch.bfloat16 and gy.is_contiguous() and x.is_contiguous()
                and gy.dim() == 2 and x.dim() == 2 and gy.shape[1] == Np and x.shape[1] == Kp and gy.shape[0] == x.shape[0]):
            return False
    return N.lib().sei_dwstream_bf16_eligible(Np, Kp, Np, Kp, *_segments(pairs)[4:]) != 0


# ---------------------------------------------------------------------------------------------
# weight gradients of the 1x1 convolutions, merged across the model calls of one step
#
# ProposedLoss calls the model twice per step (the fused SURE pass on 2B crops and the EI pass on B); each
# call's backward used to read-modify-write every weight gradient, which at the deep levels (268 M weights,
# 1.07 GB of float32 gradient each) is HBM traffic, not arithmetic. Instead the first backward to reach a
# weight parks its (gy, x) pair, and the second one issues ONE GEMM whose reduction runs over both pairs
# (sei_gemm_bf16nt_dw2). Pairs still parked when autograd finishes are flushed by an engine callback, so
# `p.grad` is complete whenever .backward() returns, whoever consumes it.
#
# "Store" mode (opt-in, GraphedLossStep): the first launch of a step into a weight gradient stores instead
# of accumulating, and zero_grad skips those gradients -- valid because the captured step writes every one
# of them exactly this way on every replay.
# ---------------------------------------------------------------------------------------------
class GradRecord:
    """What the scheduler knows about ONE gradient (`WeightGradState.records`, by data_ptr). Every field has one lifetime:

        lifetime      fields                                  set by                                 reset by
        record        ident                                   creation (WeightGradState.record)      never
        step          arrivals, written                       weight_grad16[_group], _launch         begin_step
        launch        bias                                    weight_grad16(bias=)                   the next _issue (consumes it)
        plan          numel, flops_per_row, taps, whole_step  weight_grad16[_group], _launch         weight_grad_views(reset=True)
        registration  sink, sink_launched                     set_fused_adam, set_direct_bf16_grads  the same setter

    An address met again with another shape or role -- taps or none: a freed model's tap-major gradient, now a 1x1 weight's
    -- gets a new record: nothing noted for one gradient outlives it."""

    __slots__ = ("ident", "arrivals", "written", "bias", "numel", "flops_per_row", "taps", "whole_step", "sink",
                 "sink_launched")

    def __init__(self, ident):
        self.ident = ident                              # (shape, has taps)
        self.arrivals, self.written = 0, False          # operand pairs handed in; launched into
        self.bias = None                                # bias gradient whose column sums go with the weight's next launch
        self.numel = self.flops_per_row = None          # of the view handed in; algorithmic FLOPs per reduction row to book
        self.taps = None                                # tap row offsets of a (T, N', K') gradient
        self.whole_step = False                         # its last launch was the step's complete gradient in one two-segment GEMM
        self.sink, self.sink_launched = None, False     # (kind of _SINKS, views): that launch's epilogue consumes the gradient


class WeightGradState:
    """The bookkeeping below, PER BACKBONE: model calls of the step, one `GradRecord` per gradient, parked pairs. Two
    models alive in one process (a frozen copy beside the fine-tuned one, two networks trained side by side) each merge
    and store their own weight gradients. A backbone's state is found from the address of the gradient a backward
    function writes (`register_gradient_range`: the flat gradient bucket, SwinPack's staging); gradients outside every
    registered range (kernel-level tests) share the default state. Gradients are known by their data_ptr (`key`)."""

    __slots__ = ("uses", "records", "parked", "store", "store_min", "merge", "flush_queued", "milestone", "milestone_done",
                 "dwjobs", "adamjobs", "folds", "__weakref__")

    def __init__(self):
        self.uses = 0                   # differentiated model calls of this step (note_forward)
        self.records = {}               # key -> GradRecord
        self.parked = {}                # key -> (gy16, x16, grad2d), or ("group", key) -> items: waiting for the other call
        self.store, self.store_min = False, 0   # store mode: the first launch into a gradient of >= store_min elements stores
        self.merge = True               # park and merge across the step's model calls
        self.flush_queued = False       # the engine callback of the running backward pass is queued
        self.milestone, self.milestone_done = None, False   # (frozenset of keys, event) or None (set_weight_grad_milestone)
        self.dwjobs = []                # [_Queued] for the streamed launch; their operands live until it is issued
        self.adamjobs = []              # [_QueuedAdam] for the grouped fused-Adam launch; operands live until it is issued
        self.folds = {}                 # destination pointer -> {"meta", "segs"}: deferred folds of the running pass

    def record(self, key, shape, tapped=False):
        """The record of the gradient of `shape` at `key`: a clean one unless the address is known in this shape and role."""
        rec = self.records.get(key)
        if rec is None or rec.ident != (tuple(shape), tapped):
            rec = self.records[key] = GradRecord((tuple(shape), tapped))
        return rec

    def meet(self, grad, flops_per_row=None, taps=None):
        """The record of `grad`, which a backward function hands in."""
        rec = self.record(grad.data_ptr(), grad.shape, taps is not None)
        rec.numel, rec.flops_per_row, rec.taps = grad.numel(), flops_per_row, taps
        return rec

    def set_sinks(self, kind, table):
        """Register the epilogue sinks of `kind` -- table: key -> views -- in place of those registered before."""
        for rec in self.records.values():
            if rec.sink is not None and rec.sink[0] == kind:
                rec.sink, rec.sink_launched = None, False
        if kind == SINK_ADAM:
            self.adamjobs = []          # (left behind only by a step that raised: their registration ends here)
        for key, views in (table or {}).items():
            rec = self.record(key, views[0].shape)
            rec.sink, rec.sink_launched = (kind, views), False

    def sink_launches(self, kind):
        return {k for k, r in self.records.items() if r.sink_launched and r.sink[0] == kind}

    # -- the launch decision --------------------------------------------------------------------------------
    def arrive(self, pkey, n, entry, launch):
        """The step's n-th model call brings `entry` for the gradient(s) parked under `pkey`: launched with the other call's
        entry when that waits, parked while another call is to come (and a backward pass runs to flush it), else alone."""
        partner = self.parked.pop(pkey, None)
        if partner is not None:
            launch([partner, entry])
        elif self.merge and n < self.uses and self.queue_flush():
            self.parked[pkey] = entry
        else:
            launch([entry])

    def may_store(self, grad2d):
        """This launch stores instead of accumulating: store mode, the step's first, a gradient left out of zero_grad."""
        return self.store and not self.records[grad2d.data_ptr()].written and grad2d.numel() >= self.store_min

    def whole_step(self, segments):
        """A launch over `segments` row segments carries the step's COMPLETE gradient: both model calls, merged."""
        return segments == 2 and segments == self.uses

    def _launch(self, keys, whole, issue):
        """issue() launches into the gradients `keys`, with the whole step or not; the milestone is checked even if it raises."""
        for rec in map(self.records.get, keys):
            rec.written, rec.whole_step = True, whole
        try:
            issue()
        finally:
            for key in keys:
                self.check_milestone(key)

    def launch(self, grad2d, pairs):
        store = self.may_store(grad2d)
        whole = self.whole_step(len(pairs)) and sum(gy16.shape[0] for gy16, _ in pairs) % 8 == 0   # (rows the dw2 kernels take)
        self._launch([grad2d.data_ptr()], whole, lambda: self._issue(grad2d, pairs, store))

    def _issue(self, grad2d, pairs, store):
        rec = self.records[grad2d.data_ptr()]
        # (weight_grad16(..., bias=): the bias gradient = gy's column sums rides in the streamed launch where that serves
        # the weight, else it is summed here, one column-sum launch per pair.)
        bias, rec.bias = rec.bias, None
        if bias is not None and (store or not _dwstream_ok(grad2d, pairs)):
            for gy16, _ in pairs:
                colsum16_into(bias, gy16)
            bias = None
        Np, Kp = grad2d.shape[-2:]
        g1, x1, g2, x2, K1, K2 = _segments(pairs)
        operands = (g1.data_ptr(), g2.data_ptr(), Np, x1.data_ptr(), x2.data_ptr(), Kp)
        if rec.sink is not None:
            # the update (the bf16 gradient) replaces the stored gradient only when this launch IS the step's whole gradient
            kind, views = rec.sink
            entry, what = _SINKS[kind]
            if not (store and rec.whole_step) or rec.sink_launched:
                raise RuntimeError(f"{what}: a registered weight did not receive its gradient as one merged storing GEMM "
                                   "(different loss / batch / call count than planned)")
            rec.sink_launched = True
            args = (*operands, *[N.ptr(v) for v in views], Np, Kp, K1, K2)
            if kind != SINK_ADAM or not self.queue_adam_group((g1, x1, g2, x2), views, args):
                _gemm_call(2.0 * Np * Kp * (K1 + K2), entry, *args)
            return
        taps = rec.taps
        if taps is not None:                               # (T, N', K') gradient: every tap in one launch
            T = grad2d.shape[0]
            per_row = rec.flops_per_row or 2.0 * T * Np * Kp
            if (K1 + K2) % 8 != 0:
                raise ValueError("weight_grad16 with taps: the reduction length must be a multiple of 8 rows")
            if TOKEN_STREAMING and not store and Np == 192 and Kp == 192 and T <= N.TOKGRAD_MAX_BLOCKS \
                    and K1 % 64 == 0 and K2 % 64 == 0 \
                    and g1.stride(0) == Np and x1.stride(0) == Kp and grad2d.is_contiguous():
                # 192-channel convolutions (the body of the SwinIR network): the taps are blocks of ONE token-streamed launch --
                # the same gy rows against the input rows shifted by each tap's offset, every block with its share of the CUs,
                # the two operands crossing an XCD's L2 once for all nine (sei_tokgrad_bf16_blocks; the tiled kernel re-stages
                # both operands for every 128 x 128 tile of every tap)
                blocks = [N.TokGradBlock(g1.data_ptr(), g2.data_ptr(), x1.data_ptr() + 2 * Kp * int(taps[t]),
                                         x2.data_ptr() + 2 * Kp * int(taps[t]), Np, Kp, 0, 0,
                                         grad2d.data_ptr() + 4 * t * Np * Kp, Kp) for t in range(T)]
                arr = (N.TokGradBlock * T)(*blocks)
                _gemm_call(per_row * (K1 + K2), "sei_tokgrad_bf16_blocks", arr, T, K1, K2)
                return
            _gemm_call(per_row * (K1 + K2), "sei_gemm_bf16nt_dw2_taps", *operands, grad2d.data_ptr(), Np, Kp, K1, K2,
                       int(not store), T, taps, Np * Kp)
            return
        per_row = rec.flops_per_row or 2.0 * Np * Kp
        if not store and self.queue_dwstream(grad2d, pairs, per_row, bias):
            return
        assert bias is None
        if len(pairs) == 2 and (K1 + K2) % 8 == 0:
            _gemm_call(per_row * (K1 + K2), "sei_gemm_bf16nt_dw2", *operands, grad2d.data_ptr(), Np, Kp, K1, K2, int(not store))
            return
        for gy16, x16 in pairs:
            rows = gy16.shape[0]
            if rows % 8 == 0:
                gemm_nt16(gy16, x16, Np, Kp, rows, EPI_NONE if store else EPI_ACCUM, out32=grad2d, a_rmajor=True,
                          b_rmajor=True, flops=per_row * rows)
            else:       # a pixel count the LDS-DMA kernel cannot chunk (e.g. 9 bottleneck pixels x batch 2): staged kernel
                gemm_mixed(gy16, x16, Np, Kp, rows, 1, 0, EPI_NONE if store else EPI_ACCUM, out=grad2d)
            store = False

    def launch_group(self, segs):
        """The weight gradients of several layers over the same tokens -- segs: one list of (gy16, x16, grad2d, flops per
        row) per model call of the step, the layers in the same order -- as ONE token-streamed launch
        (sei_tokgrad_bf16_blocks: every 192 x 192 block of every gradient on its share of the CUs) when the shapes allow
        it and every gradient accumulates; one launch per layer otherwise."""
        grads = [item[2] for item in segs[0]]
        rows = [seg[0][0].shape[0] for seg in segs]
        blocks, ok = [], TOKEN_STREAMING and len(segs) <= 2 and all(r % 64 == 0 for r in rows)
        for i, grad2d in enumerate(grads):
            ok = ok and grad2d.dim() == 2 and grad2d.is_contiguous() and grad2d.dtype == torch.float32
            ok = ok and not self.may_store(grad2d) and self.records[grad2d.data_ptr()].sink is None
            for s, seg in enumerate(segs):
                gy, x = seg[i][0], seg[i][1]
                ok = ok and gy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and gy.is_contiguous() and x.is_contiguous()
                ok = ok and gy.shape == (rows[s], grad2d.shape[0]) and x.shape == (rows[s], grad2d.shape[1])
            if ok:
                ok = N.lib().sei_tokgrad_bf16_eligible(grad2d.shape[0], grad2d.shape[1], grad2d.shape[0], grad2d.shape[1],
                                                       rows[0], rows[1] if len(rows) == 2 else 0) != 0
            if not ok:
                break
            Mo, Ni = grad2d.shape
            a, b = segs[0][i], segs[-1][i]
            for gy in range(Mo // 192):
                for gx in range(Ni // 192):
                    blocks.append(N.TokGradBlock(a[0].data_ptr(), b[0].data_ptr(), a[1].data_ptr(), b[1].data_ptr(), Mo, Ni,
                                                 192 * gy, 192 * gx, grad2d.data_ptr() + 4 * (192 * gy * Ni + 192 * gx), Ni))
        if not ok or len(blocks) > 8:
            for i, grad2d in enumerate(grads):
                self.launch(grad2d, [(seg[i][0], seg[i][1]) for seg in segs])
            return
        flops = sum((fpr or 2.0 * g.shape[0] * g.shape[1]) * sum(rows) for _, _, g, fpr in segs[0])
        arr = (N.TokGradBlock * len(blocks))(*blocks)
        self._launch([g.data_ptr() for g in grads], self.whole_step(len(segs)), lambda: _gemm_call(
            flops, "sei_tokgrad_bf16_blocks", arr, len(blocks), rows[0], rows[1] if len(rows) == 2 else 0))

    def check_milestone(self, key):
        ms = self.milestone
        if ms is None or key not in ms[0] or self.milestone_done:
            return
        # every gradient of the milestone has had its (single, merged) launch of this step
        if all(r is not None and r.written and r.arrivals >= max(self.uses, 1) for r in map(self.records.get, ms[0])):
            # a milestone gradient that was only QUEUED for the streamed launch (flush at the end of the backward pass)
            # must be on the stream before the event that releases it to the reducer
            if any(q.grad.data_ptr() in ms[0] for q in self.dwjobs):
                self.flush_dwstream()
            ms[1].record()
            self.milestone_done = True

    def in_early_release_range(self, ptr):
        """`ptr` lies between the gradients of the milestone: whatever is written there must be final when its event fires."""
        ms = self.milestone
        return ms is not None and min(ms[0]) <= ptr <= max(ms[0])

    # -- streamed weight gradients (DWSTREAM above) ---------------------------------------------------------
    def queue_dwstream(self, grad2d, pairs, per_row, bias=None):
        if not _dwstream_ok(grad2d, pairs):
            return False
        Np, Kp = grad2d.shape
        g1, x1, g2, x2, K1, K2 = _segments(pairs)
        job = N.DwStreamJob(g1.data_ptr(), g2.data_ptr(), x1.data_ptr(), x2.data_ptr(), Np, Kp, Np, Kp, grad2d.data_ptr(),
                            grad2d.stride(0), 0, K1, K2, N.ptr(bias))
        self.dwjobs.append(_Queued(job, (g1, x1, g2, x2, bias), grad2d, per_row * (K1 + K2)))
        if len(self.dwjobs) == N.DWSTREAM_MAX_JOBS or not self.queue_flush():
            self.flush_dwstream()
        return True

    def flush_dwstream(self):
        jobs, self.dwjobs = self.dwjobs, []
        if not jobs:
            return
        arr = (N.DwStreamJob * len(jobs))(*[q.job for q in jobs])
        _gemm_call(sum(q.flops for q in jobs), "sei_dwstream_bf16_jobs", arr, len(jobs))   # (`jobs` kept the operands alive)

    # -- grouped fused-Adam launches (ADAM_GROUP above) -----------------------------------------------------
    def queue_adam_group(self, operands, views, args):
        """Queue the fused-Adam launch with the ungrouped arguments `args` for the grouped launch; False: launch it now."""
        Np, Kp, K1, K2 = args[-4:]
        if not ADAM_GROUP or self.milestone is not None or not N.adam_gemm_groupable(Np, Kp, K1, K2):
            return False
        hyper = views[-1]
        if self.adamjobs and self.adamjobs[0].hyper is not hyper:      # one array of step scalars per launch
            self.flush_adam_group()
        if not self.queue_flush():
            return False
        g1, x1, g2, x2 = operands
        job = N.AdamGemmJob(g1.data_ptr(), g2.data_ptr(), x1.data_ptr(), x2.data_ptr(), *[N.ptr(v) for v in views[:4]],
                            Np, Kp, Np, Kp, K1, K2)
        self.adamjobs.append(_QueuedAdam(job, operands, hyper, 2.0 * Np * Kp * (K1 + K2), args))
        return True

    def flush_adam_group(self):
        jobs, self.adamjobs = self.adamjobs, []
        for i in range(0, len(jobs), N.ADAM_GROUP_MAX_JOBS):
            chunk = jobs[i:i + N.ADAM_GROUP_MAX_JOBS]               # (`jobs` keeps the operands alive until here)
            if len(chunk) == 1:
                _gemm_call(chunk[0].flops, _SINKS[SINK_ADAM][0], *chunk[0].args)
                continue
            arr = (N.AdamGemmJob * len(chunk))(*[q.job for q in chunk])
            _gemm_call(sum(q.flops for q in chunk), "sei_gemm_bf16nt_dw2_adam_group", arr, len(chunk), N.ptr(chunk[0].hyper))

    # -- deferred folds (DEFERRED_FOLDS above) --------------------------------------------------------------
    def defer_fold(self, a, b, c, ncol, split, kind, work, offset, groups):
        if not self.queue_flush():
            return False
        key = a.data_ptr()
        meta = (N.ptr(b), N.ptr(c), int(ncol), int(split), int(kind))
        job = self.folds.get(key)
        if job is not None and (job["meta"] != meta or len(job["segs"]) == 3):
            self.flush_folds()
            job = None
        if job is None:
            if len(self.folds) == N.FOLD_MAX_JOBS:
                self.flush_folds()
            job = self.folds[key] = {"meta": meta, "segs": []}       # (flush_folds starts a new table)
        job["segs"].append((work, work.data_ptr() + 4 * int(offset), int(groups)))
        return True

    def flush_folds(self):
        jobs, self.folds = self.folds, {}
        if not jobs:
            return
        arr = (N.FoldJob * len(jobs))()
        for j, (a_ptr, job) in zip(arr, jobs.items()):
            b_ptr, c_ptr, ncol, split, kind = job["meta"]
            j.a, j.b, j.c, j.ncol, j.split, j.kind, j.nseg = a_ptr, b_ptr, c_ptr, ncol, split, kind, len(job["segs"])
            for k, (_, ptr, groups) in enumerate(job["segs"]):
                j.part[k] = ptr
                j.groups[k] = groups
        N.call("sei_fold_many", arr, len(jobs))           # (the partial-sum tensors in `jobs` live until here)

    # -- the end of the backward pass -----------------------------------------------------------------------
    def queue_flush(self):
        """Ask autograd to flush parked pairs when the running backward ends; False outside a backward pass
        (then nothing may be parked: nobody would flush it)."""
        if not self.flush_queued:
            try:
                torch.autograd.Variable._execution_engine.queue_callback(self.flush)
            except RuntimeError:
                return False
            self.flush_queued = True
        return True

    def flush(self):
        """Issue every parked weight gradient on its own (no partner arrived), then the streamed jobs, the grouped fused-Adam
        launch and the folds."""
        self.flush_queued = False
        parked, self.parked = self.parked, {}
        for entry in parked.values():
            if isinstance(entry, list):                    # a parked group (weight_grad16_group)
                self.launch_group([entry])
            else:
                self.launch(entry[2], [entry[:2]])
        self.flush_dwstream()
        self.flush_adam_group()
        self.flush_folds()


_DEFAULT_STATE = WeightGradState()
_RANGES = []                      # [(first byte, end byte, weakref to the WeightGradState)], newest last


def state_of(owner=None):
    """The state of `owner` (a backbone with a flat bucket; created on first use), or the default one."""
    if owner is None:
        return _DEFAULT_STATE
    st = owner.__dict__.get("_sei_dw_state")
    if st is None:
        st = owner.__dict__["_sei_dw_state"] = WeightGradState()
    return st


def register_gradient_range(owner, tensor):
    """Gradients written inside `tensor` (the owner's flat gradient bucket, a staging buffer) belong to `owner`."""
    lo = tensor.data_ptr()
    hi = lo + tensor.numel() * tensor.element_size()
    _RANGES[:] = [r for r in _RANGES if r[2]() is not None and not (r[0] < hi and lo < r[1])]
    _RANGES.append((lo, hi, weakref.ref(state_of(owner))))


def _state_for(ptr):
    for lo, hi, ref in reversed(_RANGES):
        if lo <= ptr < hi:
            st = ref()
            if st is not None:
                return st
    return _DEFAULT_STATE


def note_forward(owner=None):
    """A model call that autograd will differentiate (ConvolutionalModel.forward / SwinIR.forward pass themselves)."""
    if torch.is_grad_enabled():
        state_of(owner).uses += 1


def begin_step(store=False, store_min=0, owner=None):
    """Start of a step (zero_grad): nothing parked, no model call counted, no gradient written yet. store: the
    first launch of the step into a weight gradient of at least store_min elements stores (it was not zeroed)."""
    st = state_of(owner)
    st.flush()
    rec = owner.__dict__.get("_sei_joint") if owner is not None else None
    if rec is not None:
        rec.reset()
    st.uses = 0
    for r in st.records.values():
        r.arrivals, r.written = 0, False
    st.milestone_done = False
    st.store, st.store_min = bool(store), int(store_min)


def set_weight_grad_merging(enabled, owner=None):
    st = state_of(owner)
    previous, st.merge = st.merge, bool(enabled)
    return previous


def weight_grad_views(reset=False, owner=None):
    """{data_ptr: numel} of every gradient view written through weight_grad16 since the last reset."""
    st = state_of(owner)
    seen = {k: r.numel for k, r in st.records.items() if r.numel is not None}
    if reset:
        for r in st.records.values():
            r.numel, r.flops_per_row, r.taps, r.whole_step = None, None, None, False
    return seen


def set_weight_grad_milestone(keys, event, owner=None):
    """Record `event` on the current stream right after the LAST of the gradients `keys` (data_ptrs) has been
    launched in a step (GraphedLossStep: an external event inside the captured backward, after which the
    bottleneck block's gradients -- most of the bucket -- are final and their all-reduce may start)."""
    state_of(owner).milestone = (frozenset(keys), event) if keys else None


def set_fused_adam(table, hyper, owner=None):
    """Optimizer step inside the weight-gradient GEMM (optim.FlatAdam.fuse_weight_updates): `table` maps the
    data_ptr of a gradient view to the (param, exp_avg, exp_avg_sq, bf16 shadow or None) views of the same shape,
    `hyper` is the device array of the step's six Adam scalars. The step's single, merged, storing launch into such a
    gradient applies the update instead of writing the gradient (sei_gemm_bf16nt_dw2_adam); None switches it off."""
    state_of(owner).set_sinks(SINK_ADAM, {k: tuple(v) + (hyper,) for k, v in table.items()} if table else None)


def set_direct_bf16_grads(table, owner=None):
    """Several GPUs, bf16-compressed exchange (parallel.FlatGradientReducer): `table` maps the data_ptr of a gradient
    view to the bf16 view of the exchange buffer with the same shape. The step's single, merged, storing launch into
    such a gradient writes bf16 there (sei_gemm_bf16nt_dw2_bf16out) and nothing into the float32 bucket, which the
    reducer then does not cast for those ranges; None switches it off."""
    state_of(owner).set_sinks(SINK_BF16, {k: (v,) for k, v in table.items()} if table else None)


def direct_bf16_launches(owner=None):
    return state_of(owner).sink_launches(SINK_BF16)


def fused_adam_launches(owner=None):
    """data_ptrs whose update was applied inside a GEMM since set_fused_adam."""
    return state_of(owner).sink_launches(SINK_ADAM)


def merged_weight_grads(owner=None):
    """data_ptrs of the gradients whose last launch carried the step's COMPLETE gradient as one two-segment GEMM (the
    condition for applying the optimizer step, or writing bf16, in that launch: graphs.GraphedLossStep reads this after
    its warm-up steps -- a batch whose pixel counts do not add up to a multiple of 8 rows is served by other launches)."""
    return {k for k, r in state_of(owner).records.items() if r.whole_step}


def flush_weight_grads(owner=None):
    """Issue every parked weight gradient of `owner` (default state when None) on its own (no partner arrived)."""
    state_of(owner).flush()


def weight_grad16(gy16, x16, grad2d, flops_per_row=None, tap_rows=None, bias=None):
    """grad (N', K') += gy^T x, gy16 (M, N') and x16 (M, K') bf16 as stored: both read reduction-major.
    May park the pair until the step's other model call reaches the same weight (see above). flops_per_row: the
    algorithmic FLOPs per reduction row to book for the roofline leg when the operands are zero-padded (2 N' K').
    tap_rows (a ctypes int array of T row offsets): grad2d is (T, N', K') and slice t is gy^T x[rows shifted by
    tap_rows[t]] -- the taps of a 3x3 convolution's weight gradient in one launch (sei_gemm_bf16nt_dw2_taps); x16 is
    the un-shifted window of a grid with guard rows on both sides."""
    key = grad2d.data_ptr()
    st = _state_for(key)
    rec = st.meet(grad2d, flops_per_row, tap_rows)
    if bias is not None:                   # (M,)-shaped float32 gradient: += gy's column sums, with the weight's launch
        rec.bias = bias
    split = _gemm._JOINT_SPLIT
    if split is not None and tap_rows is None:
        # one backward pass for the step's two model calls (models/_joint.py): the operands hold both calls' rows -- the
        # two row segments that two backward functions would otherwise have brought one after the other
        M1 = gy16.shape[0] * split[0] // (split[0] + split[1])
        rec.arrivals += 2
        st.launch(grad2d, [(gy16[:M1], x16[:M1]), (gy16[M1:], x16[M1:])])
        return
    rec.arrivals += 1
    st.arrive(key, rec.arrivals, (gy16, x16, grad2d), lambda entries: st.launch(grad2d, [e[:2] for e in entries]))


def weight_grad16_group(items):
    """weight_grad16 for several layers whose operands cover the SAME tokens (the four linear layers of a Swin block):
    items = [(gy16, x16, grad2d, flops_per_row)]. Parked and merged across the step's model calls like single pairs; the
    launch is one token-streamed kernel for all of them (WeightGradState.launch_group)."""
    items = list(items)
    head = items[0][2].data_ptr()
    st = _state_for(head)
    for _, _, grad2d, fpr in items:
        st.meet(grad2d, fpr).arrivals += 1
    st.arrive(("group", head), st.records[head].arrivals, items, st.launch_group)


def defer_fold(a, b, c, ncol, split, kind, work, offset, groups):
    """Register `work[offset:]` ([groups][ncol] partial sums, kept alive here) to be folded into a (| b | c) when the
    running backward pass ends. False: not deferred (switched off / no backward pass running) -- the caller folds."""
    return DEFERRED_FOLDS and _state_for(a.data_ptr()).defer_fold(a, b, c, ncol, split, kind, work, offset, groups)
