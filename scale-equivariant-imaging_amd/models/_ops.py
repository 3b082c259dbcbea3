"""Autograd functions of the U-Net blocks, each a short sequence of HIP kernel launches.

Activations are NHWC float32 tensors (B, H, W, C); a 1x1 convolution is then a row-major GEMM over
the (B*H*W, C) view. Parameter gradients are not returned to autograd: every backward ACCUMULATES
straight into `param.grad` (a view of the model's flat gradient bucket when the model has been
flattened), which is what lets the kernels fuse "grad += ..." and keeps one contiguous buffer for the
fused Adam step and the RCCL all-reduce. `optimizer.zero_grad()` (either flavour) is honoured.
"""
import os

import torch

import _native as N
from . import _mats, _wgrad
# (the GEMM dispatch, the cached bf16 weight copies and the weight-gradient scheduler are modules of their own; the names
# the rest of the package, the tests and the tools reach through this module are imported here. The switches DWSTREAM,
# DEFERRED_FOLDS and TOKEN_STREAMING are read where they live, models/_wgrad.py: assign them there)
from ._gemm import (EPI_ACCUM, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_BIAS_ROWSCALE, EPI_MUL_DGELU, EPI_NONE,  # noqa: F401
                    SPLITK_COUNTER_BYTES, SPLITK_WS_MIB, SPLITK_WS_STREAMS, _SPLITK_WS, _gemm_call, _in_forward_mode,
                    compute_dtype_scope, gemm, gemm_mixed, gemm_nt16, gemm_x3, get_compute_dtype, joint_rows,
                    own_splitk_workspace, profile_gemms, release_splitk_workspace, reset_splitk_counters, set_compute_dtype,
                    splitk_workspace)
from ._joint import JointCtx, _NotJoint, joint_ctx, walk_backward  # noqa: F401
from ._shadow import (ShadowState, _new_plain_state, _transposed16, _transposed16_cached, plain_shadow_is_current,  # noqa: F401
                      refresh_plain_shadow, set_stale_masters, shadow, split_x2, weights_updated)
from ._wgrad import (_state_for, begin_step, colsum16_into, defer_fold, direct_bf16_launches, flush_weight_grads,  # noqa: F401
                     fused_adam_launches, merged_weight_grads, note_forward, register_gradient_range,
                     set_direct_bf16_grads, set_fused_adam, set_weight_grad_merging, set_weight_grad_milestone, state_of,
                     weight_grad16, weight_grad16_group, weight_grad_views)

LN_EPS = 1e-6


# ---------------------------------------------------------------------------------------------
# gradient buckets
# ---------------------------------------------------------------------------------------------
def grad_of(p):
    """The tensor to accumulate p's gradient into (zeroed on first touch after zero_grad)."""
    if p.grad is None:
        view = getattr(p, "_sei_grad_view", None)
        if view is None or view.shape != p.shape or view.device != p.device:
            view = torch.zeros_like(p, memory_format=torch.contiguous_format)
        else:
            view.zero_()
        p.grad = view
    return p.grad


# ---------------------------------------------------------------------------------------------
# activations of a RECORDED model call come from the recorder's arena (models/_joint.py: the step's two model calls
# share one backward pass over 3B-row tensors); everything else is torch.empty
# ---------------------------------------------------------------------------------------------
_ARENA = None            # the models._joint.Recorder of the model call being recorded, or None


def _alloc(shape, dtype, device):
    if _ARENA is None:
        return torch.empty(tuple(shape), dtype=dtype, device=device)
    return _ARENA.alloc(shape, dtype, device)


def _tape(fn, ctx):
    if _ARENA is not None:
        _ARENA.record(fn, ctx)


def _no_joint_form():
    """Called by layer functions that have no joint backward (the float32 path, stand-alone resamplers / LayerNorms)."""
    if _ARENA is not None:
        _ARENA.unsupported()


class recording:
    """`with recording(recorder):` around a model call: its layer functions allocate from the arena and fill the tape."""

    def __init__(self, rec):
        self.rec = rec

    def __enter__(self):
        global _ARENA
        self.prev, _ARENA = _ARENA, self.rec
        return self.rec

    def __exit__(self, *exc):
        global _ARENA
        _ARENA = self.prev
        return False


# ---------------------------------------------------------------------------------------------
# thin launch helpers (pointers + sizes only; shapes are checked here, on the host)
# ---------------------------------------------------------------------------------------------
def layer_norm(x2d, gamma, beta):
    rows, C = x2d.shape
    y = _alloc((rows, C), torch.float32, x2d.device)
    mean = _alloc((rows,), torch.float32, x2d.device)
    rstd = _alloc((rows,), torch.float32, x2d.device)
    N.call("sei_ln_fwd", x2d.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(),
           rstd.data_ptr(), rows, C, LN_EPS)
    return y, mean, rstd


def layer_norm_bwd(x2d, gamma, mean, rstd, gy, ggamma, gbeta, res=None):
    """res: a second gradient of the LayerNorm's input (rows, C), added to gx in the same kernel (the skip connection's
    gradient where a level's output feeds the downsampler and the decoder: no autograd add kernel)."""
    rows, C = x2d.shape
    gx = torch.empty_like(x2d)
    need = N.lib().sei_ln_bwd_workspace(rows, C)
    work = torch.empty(max(need, 1), dtype=torch.float32, device=x2d.device)
    parts = N.lib().sei_ln_bwd_part_count(rows, C)
    deferred = parts > 0 and defer_fold(ggamma, gbeta, None, 2 * C, C, N.FOLD_SPLIT, work,
                                        N.lib().sei_ln_bwd_part_offset(rows, C), parts)
    fused_res = res is not None and parts > 0
    N.call("sei_ln_bwd_res", x2d.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gy.data_ptr(),
           res.data_ptr() if fused_res else None, gx.data_ptr(), None if deferred else ggamma.data_ptr(),
           None if deferred else gbeta.data_ptr(), rows, C, work.data_ptr(), need)
    if res is not None and not fused_res:
        gx += res.view(rows, C)
    return gx


def colsum_into(acc, x2d, row_weight=None):
    """acc[n] += sum_m x2d[m, n] (times row_weight[m] if given): a bias gradient. The kernels take a pointer and (M, N):
    rows N floats apart, N accumulators, M weights. Anything else (a column slice of a wider matrix, an accumulator of
    another length) is refused here: the kernels would sum, or add to, other memory."""
    M, Nn = x2d.shape
    if not x2d.is_contiguous() or not acc.is_contiguous() or acc.numel() != Nn:
        raise ValueError(f"colsum_into: expected contiguous (M, N) rows and N contiguous accumulators, got rows of shape "
                         f"{tuple(x2d.shape)} and strides {x2d.stride()}, accumulators of shape {tuple(acc.shape)}")
    if row_weight is not None and (not row_weight.is_contiguous() or row_weight.numel() != M):
        raise ValueError(f"colsum_into: expected {M} contiguous row weights, got shape {tuple(row_weight.shape)}")
    if row_weight is None:
        N.call("sei_colsum_f32", x2d.data_ptr(), acc.data_ptr(), M, Nn)
    else:
        N.call("sei_colsum_weighted_f32", x2d.data_ptr(), row_weight.data_ptr(), acc.data_ptr(), M, Nn)


def dwconv7(x, w, bias, flip=False, res=None, res_scale=1.0, seg=0):
    """seg > 0: the generic kernels with that segment width (sei_dwconv7_fwd_ex; tests), 0 = chosen by shape."""
    B, H, W, C = x.shape
    y = torch.empty_like(x)
    args = (x.data_ptr(), w.data_ptr(), N.ptr(bias), N.ptr(res), float(res_scale), y.data_ptr(), B, H, W, C, int(flip))
    if seg:
        N.call("sei_dwconv7_fwd_ex", *args, int(seg))
    else:
        N.call("sei_dwconv7_fwd", *args)
    return y


def dwconv7_ln(x, w, bias, gamma, beta, out16, fuse=0):
    """ConvBlock.conv1 -> LayerNorm (reference convolutional.py:36-39) through sei_dwconv7_ln_fwd: one fused launch
    at the first level (C = 32), the depthwise kernel + the stand-alone LayerNorm elsewhere (fuse: 1 / 2 force either
    form; tests). Returns h1 (f32, NHWC), h2 ((M, C) bf16 when out16 else f32), mean, rstd."""
    B, H, W, C = x.shape
    M = B * H * W
    h1 = _alloc((B, H, W, C), torch.float32, x.device)
    h2 = _alloc((M, C), torch.bfloat16 if out16 else torch.float32, x.device)
    mean = _alloc((M,), torch.float32, x.device)
    rstd = _alloc((M,), torch.float32, x.device)
    args = (x.data_ptr(), w.data_ptr(), N.ptr(bias), gamma.data_ptr(), beta.data_ptr(), h1.data_ptr(), h2.data_ptr(),
            int(out16), mean.data_ptr(), rstd.data_ptr(), B, H, W, C, LN_EPS)
    if fuse:
        N.call("sei_dwconv7_ln_fwd_ex", *args, int(fuse))
    else:
        N.call("sei_dwconv7_ln_fwd", *args)
    return h1, h2, mean, rstd


def dwconv7_weight_grad(x, gy, gw, gb, seg=0):
    B, H, W, C = x.shape
    need = N.lib().sei_dwconv7_bwd_weight_workspace_ex(B, H, W, C, int(seg))
    work = torch.empty(need, dtype=torch.float32, device=x.device)
    deferred = need > 0 and defer_fold(gw, gb, None, 50 * C, C, N.FOLD_DWCONV7, work, 0, need // (50 * C))
    N.call("sei_dwconv7_bwd_weight_ex", x.data_ptr(), gy.data_ptr(), None if deferred else gw.data_ptr(),
           None if deferred else N.ptr(gb), B, H, W, C, work.data_ptr(), need, int(seg))


def sepmap2(x, mats, Ho, Wo):
    """mats: (L1, R1, L2, R2[, RW, LH]) -- the packed pair comes with `_mats.resample_matrices`; a bare 4-tuple
    (tests, experiments) is packed here."""
    B, Hi, Wi, C = x.shape
    y = _alloc((B, Ho, Wo, C), torch.float32, x.device)
    work = torch.empty(2 * B * Hi * Wo * C, dtype=torch.float32, device=x.device)
    RW, LH = (mats[4], mats[5]) if len(mats) >= 6 else _mats.pack_for_kernel(mats[:4], x.device)
    N.call("sei_sepmap2_packed", x.data_ptr(), y.data_ptr(), B, Hi, Wi, Ho, Wo, C, RW.data_ptr(), LH.data_ptr(),
           work.data_ptr(), work.numel())
    return y


def sepmap2_16(x, mats, Ho, Wo, out16=False):
    """sepmap2 in the bf16 throughput mode: on the matrix cores where the shape is eligible (sei_sepmap2_bf16:
    activations rounded to bf16, matrices as bf16 head + remainder, f32 accumulation), else the f32 kernels.
    out16: the caller wants the result as a bf16 GEMM operand; the kernels that can write it directly (the one-pass kernel of
    the deepest levels, the matrix-core kernel of the 24 - 64-pixel extents) return a bfloat16 tensor -- the float32
    accumulator rounded once, exactly what a cast pass would have produced -- the others float32 (the caller casts)."""
    B, Hi, Wi, C = x.shape
    if x.is_cuda and N.lib().sei_sepmap2_small_eligible(B, Hi, Wi, Ho, Wo, C):
        # the deep levels' 6- and 3-pixel images: one float32 pass through LDS, no HBM intermediate (round 5)
        y = _alloc((B, Ho, Wo, C), torch.bfloat16 if out16 else torch.float32, x.device)
        L1, R1, L2, R2 = mats[:4]
        N.call("sei_sepmap2_small", x.data_ptr(), y.data_ptr(), int(out16), B, Hi, Wi, Ho, Wo, C, L1.data_ptr(),
               R1.data_ptr(), L2.data_ptr(), R2.data_ptr())
        return y
    small = x.is_cuda and max(Hi, Wi, Ho, Wo) <= 64 and N.lib().sei_sepmap2_bf16_eligible(B, Hi, Wi, Ho, Wo, C)
    big = not small and x.is_cuda and N.lib().sei_sepmap2_big_eligible(B, Hi, Wi, Ho, Wo, C)
    if not big and x.is_cuda and N.lib().sei_sepmap2_bf16_eligible(B, Hi, Wi, Ho, Wo, C):
        y = _alloc((B, Ho, Wo, C), torch.bfloat16 if out16 else torch.float32, x.device)
        N.call("sei_sepmap2_bf16_out16" if out16 else "sei_sepmap2_bf16", x.data_ptr(), y.data_ptr(), B, Hi, Wi, Ho, Wo, C,
               _packed16(mats).data_ptr())
        return y
    if big:
        # extents beyond one workgroup's LDS (the x4 network's 96- / 192-pixel levels, 256-pixel inputs): two launches of
        # the constant-matrix GEMM kernel with a bf16 intermediate
        y = _alloc((B, Ho, Wo, C), torch.float32, x.device)
        work = torch.empty(N.lib().sei_sepmap2_big_work_elems(B, Hi, Wi, Ho, Wo, C), dtype=torch.int16, device=x.device)
        N.call("sei_sepmap2_big", x.data_ptr(), y.data_ptr(), B, Hi, Wi, Ho, Wo, C, _packed16(mats, big=True).data_ptr(),
               work.data_ptr())
        return y
    return sepmap2(x, mats, Ho, Wo)


_PACKED16 = {}


def _packed16(mats, big=False):
    """The map's matrices in sei_sepmap2_bf16's (big: sei_sepmap2_big's) image (bf16 head + remainder), packed once per
    matrix set."""
    L1, R1, L2, R2 = mats[:4]
    key = (L1.data_ptr(), R1.data_ptr(), L2.data_ptr(), R2.data_ptr(), tuple(L1.shape), tuple(R1.shape), big)
    hit = _PACKED16.get(key)
    if hit is None:
        (Ho, Hi), (Wo, Wi) = L1.shape, R1.shape
        kind = "sei_sepmap2_big" if big else "sei_sepmap2_bf16"
        out = torch.empty(getattr(N.lib(), kind + "_pack_elems")(Hi, Wi, Ho, Wo), dtype=torch.int16, device=L1.device)
        N.call(kind + "_pack", L1.data_ptr(), R1.data_ptr(), L2.data_ptr(), R2.data_ptr(), out.data_ptr(), Hi, Wi,
               Ho, Wo)
        hit = _PACKED16[key] = (out, L1, R1, L2, R2)          # (keeps the sources alive: the key holds their addresses)
    return hit[0]


def _nhwc(x):
    N.check_tensor(x, "activation")
    if x.dim() != 4:
        raise ValueError("expected an NHWC activation (B, H, W, C)")
    return x


# ---------------------------------------------------------------------------------------------
# ConvBlock: x + conv3(gelu(conv2(LN(dwconv7(x)))))   (reference convolutional.py:33-51)
# `twice` adds the block input a second time: the encoder's inner residual x + xb with xb == x
# (convolutional.py:226-231) fused into the last GEMM's epilogue.
# ---------------------------------------------------------------------------------------------
def _convblock_tail(ctx, x, h1, mean, rstd, gh2, go):
    """The end of every ConvBlock backward, from the gradient gh2 of the LayerNorm's output: LayerNorm backward, depthwise
    weight gradient, flipped depthwise data gradient with the residual's `go` (twice over when the block input was added
    twice) in its epilogue."""
    w1, b1, gamma, beta = ctx.params[:4]
    B, H, W, C = x.shape
    gh1 = layer_norm_bwd(h1.view(B * H * W, C), gamma, mean, rstd, gh2, grad_of(gamma), grad_of(beta)).view(B, H, W, C)
    dwconv7_weight_grad(x, gh1, grad_of(w1), grad_of(b1))
    gx = None
    if ctx.needs_input_grad[0]:
        gx = dwconv7(gh1, w1, None, flip=True, res=go, res_scale=2.0 if ctx.twice else 1.0)
    return (gx,) + (None,) * 9


class ConvBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, gamma, beta, w2, b2, w3, b3, twice):
        _no_joint_form()
        ctx.dtype = get_compute_dtype()
        x = _nhwc(x)
        B, H, W, C = x.shape
        M = B * H * W
        h1, h2, mean, rstd = dwconv7_ln(x, w1, b1, gamma, beta, out16=False)
        h4 = torch.empty((M, 4 * C), dtype=torch.float32, device=x.device)
        h3 = gemm(h2, w2, M, 4 * C, C, 0, 1, EPI_BIAS_GELU, bias=b2, D2=h4)
        out = gemm(h4, w3, M, C, 4 * C, 0, 1, EPI_BIAS_RES, bias=b3, R1=x, R2=x if twice else None)
        ctx.save_for_backward(x, h1, mean, rstd, h2, h3, h4)
        ctx.params = (w1, b1, gamma, beta, w2, b2, w3, b3)
        ctx.twice = twice
        return out.view(B, H, W, C)

    @_in_forward_mode
    def backward(ctx, go):
        x, h1, mean, rstd, h2, h3, h4 = ctx.saved_tensors
        w1, b1, gamma, beta, w2, b2, w3, b3 = ctx.params
        B, H, W, C = x.shape
        M = B * H * W
        go = go.contiguous()
        go2 = go.view(M, C)
        # conv3
        colsum_into(grad_of(b3), go2)
        gemm(go2, h4, C, 4 * C, M, 1, 0, EPI_ACCUM, out=grad_of(w3).view(C, 4 * C))
        gh3 = gemm(go2, w3, M, 4 * C, C, 0, 0, EPI_MUL_DGELU, R1=h3)          # (go W3) * gelu'(h3)
        # conv2
        colsum_into(grad_of(b2), gh3)
        gemm(gh3, h2, 4 * C, C, M, 1, 0, EPI_ACCUM, out=grad_of(w2).view(4 * C, C))
        gh2 = gemm(gh3, w2, M, C, 4 * C, 0, 0, EPI_NONE)
        return _convblock_tail(ctx, x, h1, mean, rstd, gh2, go)


# ---------------------------------------------------------------------------------------------
# What the float32 and the bf16 class of a resampling layer share: shapes and matrices, the skip check, and the end of
# the backward. `resample` is the class's own resampler (sepmap2 / sepmap2_16); the other launches are the same for both.
# ---------------------------------------------------------------------------------------------
def _resample_prologue(kind, x, w, rate):
    """(B, H, W, C, Co, fwd, bwd, Ho, Wo) of a resampling layer on the NHWC input x with the 1x1 weight w."""
    B, H, W, C = x.shape
    fwd, bwd = _mats.resample_matrices(kind, H, W, rate, x.device)
    return B, H, W, C, w.shape[0], fwd, bwd, fwd[0].shape[0], fwd[1].shape[0]


def _downsample_tail(ctx, gu, gskip, resample):
    """From the gradient gu (Mo, C) of the resampler's output: its adjoint, then the LayerNorm backward with the skip
    connection's gradient added in the same kernel."""
    x, mean, rstd = ctx.saved_tensors[:3]
    gamma, beta = ctx.params[:2]
    B, H, W, C = x.shape
    M = B * H * W
    gh = resample(gu.view(B, ctx.hw[2], ctx.hw[3], C), ctx.mats_t, H, W).view(M, C)
    res = None if gskip is None else gskip.contiguous().view(M, C)
    gx = layer_norm_bwd(x.view(M, C), gamma, mean, rstd, gh, grad_of(gamma), grad_of(beta), res=res).view(B, H, W, C)
    return (gx if ctx.needs_input_grad[0] else None), None, None, None, None, None, None


def _check_skip(skip, shape):
    skip = _nhwc(skip)
    if tuple(skip.shape) != shape:
        raise ValueError("skip connection shape mismatch")
    return skip


def _upsample_tail(ctx, go, gh, resample):
    """From the gradient gh (M, C) of the LayerNorm's output: LayerNorm backward, the resampler's adjoint; the skip
    connection's gradient is `go` itself."""
    u, mean, rstd = ctx.saved_tensors[:3]
    gamma, beta = ctx.params[:2]
    gu = layer_norm_bwd(u.view(-1, u.shape[-1]), gamma, mean, rstd, gh, grad_of(gamma), grad_of(beta))
    gx = None
    if ctx.needs_input_grad[0]:
        gx = resample(gu.view(u.shape), ctx.mats_t, *ctx.in_hw)
    gskip = go if ctx.needs_input_grad[1] else None
    return gx, gskip, None, None, None, None, None


# ---------------------------------------------------------------------------------------------
# Downsample: LN -> 1x1 conv C -> 4C -> ideal downsample    (reference convolutional.py:136-150)
# ---------------------------------------------------------------------------------------------
class DownsampleFn(torch.autograd.Function):
    """LN -> 1x1 conv C->Co -> ideal downsample, evaluated as LN -> ideal downsample -> 1x1 conv.

    The resampler is linear and acts per channel, the convolution is linear and acts per pixel, so they
    commute exactly; only the bias needs care: it comes out of the resampler as bias[c] * s[pixel], s = the
    resampler's response to a constant image (`_mats.constant_response`), which is the BIAS_ROWSCALE epilogue.
    The resampler then runs on C channels instead of Co = 4C, the three GEMMs on a quarter of the rows, and the
    full-resolution Co-channel tensor (75 MB per level at B = 32) never exists."""

    @staticmethod
    def forward(ctx, x, gamma, beta, w, b, rate, with_skip=False):
        """with_skip: also return x itself as a second output (the U-Net's skip connection): its gradient then arrives
        HERE, next to the downsampler's, and is added inside the LayerNorm backward instead of by an autograd add."""
        _no_joint_form()
        ctx.dtype = get_compute_dtype()
        ctx.set_materialize_grads(False)
        x = _nhwc(x)
        h, mean, rstd = layer_norm(x.view(-1, x.shape[-1]), gamma, beta)
        B, H, W, C, Co, fwd, bwd, Ho, Wo = _resample_prologue("down", x, w, rate)
        u = sepmap2(h.view(B, H, W, C), fwd, Ho, Wo)
        Mo = B * Ho * Wo
        s = _mats.constant_response("down", H, W, rate, x.device, B)
        out = gemm(u.view(Mo, C), w, Mo, Co, C, 0, 1, EPI_BIAS_ROWSCALE, bias=b, R1=s)
        ctx.save_for_backward(x, mean, rstd, u, s)
        ctx.params, ctx.mats_t, ctx.hw = (gamma, beta, w, b), bwd, (H, W, Ho, Wo)
        out = out.view(B, Ho, Wo, Co)
        return (out, x) if with_skip else out

    @_in_forward_mode
    def backward(ctx, go, gskip=None):
        x, mean, rstd, u, s = ctx.saved_tensors
        gamma, beta, w, b = ctx.params
        Mo, (Co, C) = x.shape[0] * ctx.hw[2] * ctx.hw[3], w.shape[:2]
        go2 = go.contiguous().view(Mo, Co)
        colsum_into(grad_of(b), go2, row_weight=s)
        gemm(go2, u.view(Mo, C), Co, C, Mo, 1, 0, EPI_ACCUM, out=grad_of(w).view(Co, C))
        gu = gemm(go2, w, Mo, C, Co, 0, 0, EPI_NONE)
        return _downsample_tail(ctx, gu, gskip, sepmap2)


# ---------------------------------------------------------------------------------------------
# Upsample: ideal upsample -> LN -> 1x1 conv (+ skip)       (reference convolutional.py:95-110,236-240)
# ---------------------------------------------------------------------------------------------
class UpsampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, skip, gamma, beta, w, b, rate):
        _no_joint_form()
        ctx.dtype = get_compute_dtype()
        x = _nhwc(x)
        B, H, W, C, Co, fwd, bwd, Ho, Wo = _resample_prologue("up", x, w, rate)
        u = sepmap2(x, fwd, Ho, Wo)
        M = B * Ho * Wo
        h, mean, rstd = layer_norm(u.view(M, C), gamma, beta)
        if skip is not None:
            out = gemm(h, w, M, Co, C, 0, 1, EPI_BIAS_RES, bias=b, R1=_check_skip(skip, (B, Ho, Wo, Co)))
        else:
            out = gemm(h, w, M, Co, C, 0, 1, EPI_BIAS, bias=b)
        ctx.save_for_backward(u, mean, rstd, h)
        ctx.params, ctx.mats_t, ctx.in_hw = (gamma, beta, w, b), bwd, (H, W)
        return out.view(B, Ho, Wo, Co)

    @_in_forward_mode
    def backward(ctx, go):
        u, mean, rstd, h = ctx.saved_tensors
        gamma, beta, w, b = ctx.params
        B, Ho, Wo, C = u.shape
        M, Co = B * Ho * Wo, w.shape[0]
        go = go.contiguous()
        go2 = go.view(M, Co)
        colsum_into(grad_of(b), go2)
        gemm(go2, h, Co, C, M, 1, 0, EPI_ACCUM, out=grad_of(w).view(Co, C))
        gh = gemm(go2, w, M, C, Co, 0, 0, EPI_NONE)
        return _upsample_tail(ctx, go, gh, sepmap2)


# =============================================================================================
# bf16 throughput mode (--compute_dtype bf16): GEMM-only activations are STORED in bf16, weights get
# bf16 shadows (plain + transposed) refreshed once per optimizer step, and every GEMM whose operands can
# be K-contiguous runs on the direct-to-LDS kernel (sei_gemm_bf16nt). Weight gradients use the
# register-staged kernel on the bf16 tensors and accumulate into the f32 gradient bucket. Everything
# else (depthwise conv, LayerNorm statistics and backward, resamplers, residuals, Adam) stays f32.
# =============================================================================================
def nt16_ok(K):
    return K % 8 == 0


def to_bf16(x):
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    N.call("sei_cast_bf16", x.data_ptr(), y.data_ptr(), x.numel())
    return y


def layer_norm16(x2d, gamma, beta):
    rows, C = x2d.shape
    y = _alloc((rows, C), torch.bfloat16, x2d.device)
    mean = _alloc((rows,), torch.float32, x2d.device)
    rstd = _alloc((rows,), torch.float32, x2d.device)
    N.call("sei_ln_fwd_bf16", x2d.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(),
           rstd.data_ptr(), rows, C, LN_EPS)
    return y, mean, rstd


def cast16(x2d, colsum_into_=None, row_weight=None):
    """f32 (R, C) -> bf16 copy; colsum_into_: accumulate the column sums (a bias gradient) in the same pass, each row
    times row_weight[r] when given (the downsampler's convolution: DownsampleFn16)."""
    R, C = x2d.shape
    x16 = _alloc((R, C), torch.bfloat16, x2d.device)
    if colsum_into_ is not None and C % 4 == 0:
        # the column sums leave as per-row-block partial sums and join the pass's deferred folds (no atomics: the grid is
        # sized for bandwidth); outside a backward pass the atomics form below
        parts = N.lib().sei_cast_bf16_colsum_parts_count(R, C)
        # (a bias gradient between the two early-released weight gradients must be final when their event fires: such a
        # destination -- none in the U-Net, whose only bias there comes from a GEMM epilogue -- keeps the atomics)
        early = _state_for(colsum_into_.data_ptr()).in_early_release_range(colsum_into_.data_ptr())
        if parts > 0 and not early:
            work = torch.empty(parts * C, dtype=torch.float32, device=x2d.device)
            if defer_fold(colsum_into_, None, None, C, C, N.FOLD_SPLIT, work, 0, parts):
                N.call("sei_cast_bf16_colsum_parts", x2d.data_ptr(), x16.data_ptr(), N.ptr(row_weight), work.data_ptr(), R, C)
                return x16
    if row_weight is not None and colsum_into_ is not None and C % 4 == 0:
        N.call("sei_cast_bf16_colsum_weighted", x2d.data_ptr(), x16.data_ptr(), row_weight.data_ptr(), colsum_into_.data_ptr(),
               R, C)
        return x16
    if row_weight is not None and colsum_into_ is not None:
        colsum_into(colsum_into_, x2d, row_weight=row_weight)
        colsum_into_ = None
    N.call("sei_cast_transpose_bf16", x2d.data_ptr(), 0, x16.data_ptr(), None, R, C, R, N.ptr(colsum_into_))
    return x16


def use_bf16_blocks(C):
    """A block takes the bf16-storage path when the mode is bf16 and its GEMMs fit the NT kernel."""
    return get_compute_dtype() == "bf16" and C % 32 == 0


# Levels whose ConvBlock MLP runs as the fused kernel. Measured on MI355X at batch 32 (2B pass): C = 32 wins
# (forward 40 vs 56 us for the two GEMMs, backward 49 vs 76 us incl. the cast); C = 128 loses (forward 63 vs 51 us,
# backward 139 vs 70 us): 36,864 pixels are 288 four-wave tiles, one per CU, and nothing overlaps the 16 serial
# weight slices of a tile. SEI_FUSED_MLP=32,128 / SEI_FUSED_MLP= (empty) override for A/B runs.
# Round 4: the 128-channel level has a kernel of its own (csrc/mlp128.hip: nine-wave workgroups of 144 pixels, weights
# through an LDS-DMA ring) for pixel counts that are multiples of 144 -- sei_mlp_fused_eligible says where the fused form is
# the faster one; everything else keeps the GEMMs.
FUSED_MLP_CHANNELS = tuple(int(v) for v in os.environ.get("SEI_FUSED_MLP", "32,128").split(",") if v)


def fused_mlp_ok(M, C):
    return C in FUSED_MLP_CHANNELS and N.lib().sei_mlp_fused_eligible(M, C) != 0


class ConvBlockFn16(torch.autograd.Function):
    """ConvBlockFn with bf16 storage of h2 / h4 / gh3 and the direct-to-LDS GEMMs (C % 32 == 0: `use_bf16_blocks`). At
    the shallow levels (C in FUSED_MLP_CHANNELS) conv2 -> GELU -> conv3 + residual is ONE launch whose 4C-wide hidden
    activation never reaches HBM (sei_mlp_fused_fwd); the backward recomputes it (sei_mlp_fused_bwd)."""

    @staticmethod
    def forward(ctx, x, w1, b1, gamma, beta, w2, b2, w3, b3, twice):
        ctx.dtype = get_compute_dtype()
        x = _nhwc(x)
        B, H, W, C = x.shape
        M = B * H * W
        h1, h2, mean, rstd = dwconv7_ln(x, w1, b1, gamma, beta, out16=True)
        w2_16, w3_16 = shadow(w2), shadow(w3)
        ctx.fused = fused_mlp_ok(M, C)
        _tape(ConvBlockFn16, ctx)
        if ctx.fused:
            out = _alloc((M, C), torch.float32, x.device)
            # counted with the GEMM family (roofline leg): 2 GEMMs of M x 4C x C
            _gemm_call(4.0 * M * 4 * C * C, "sei_mlp_fused_fwd", h2.data_ptr(), w2_16.data_ptr(), b2.data_ptr(),
                       w3_16.data_ptr(), b3.data_ptr(), x.data_ptr(), 2.0 if twice else 1.0, out.data_ptr(), M, C)
            saved = (x, h1, mean, rstd, h2)
        else:
            h3 = _alloc((M, 4 * C), torch.float32, x.device)
            h4 = _alloc((M, 4 * C), torch.bfloat16, x.device)
            gemm_nt16(h2, w2_16, M, 4 * C, C, EPI_BIAS_GELU, out32=h3, bias=b2, D2_16=h4)
            out = _alloc((M, C), torch.float32, x.device)
            gemm_nt16(h4, w3_16, M, C, 4 * C, EPI_BIAS_RES, out32=out, bias=b3, R1=x, R2=x if twice else None)
            saved = (x, h1, mean, rstd, h2, h3, h4)
        ctx.save_for_backward(*saved)
        ctx.params = (w1, b1, gamma, beta, w2, b2, w3, b3)
        ctx.twice = twice
        return out.view(B, H, W, C)

    @_in_forward_mode
    def backward(ctx, go):
        if ctx.fused:
            return ConvBlockFn16._backward_fused(ctx, go)
        x, h1, mean, rstd, h2, h3, h4 = ctx.saved_tensors
        w1, b1, gamma, beta, w2, b2, w3, b3 = ctx.params
        B, H, W, C = x.shape
        M = B * H * W
        go = go.contiguous()
        go2 = go.view(M, C)
        # Each weight's data gradient goes BEFORE its weight gradient: with the optimizer step fused into the weight-
        # gradient GEMM (set_fused_adam) that launch rewrites the weight's bf16 shadow, which the data gradient reads.
        go16 = cast16(go2, colsum_into_=grad_of(b3))
        gh3 = torch.empty((M, 4 * C), dtype=torch.bfloat16, device=x.device)
        # (go W3) gelu'(h3), with conv2's bias gradient = its column sums riding in the epilogue (no pass over gh3)
        gemm_nt16(go16, shadow(w3), M, 4 * C, C, EPI_MUL_DGELU, out16=gh3, R1=h3, b_rmajor=True, colsum=grad_of(b2))
        weight_grad16(go16, h4, grad_of(w3).view(C, 4 * C))
        gh2 = torch.empty((M, C), dtype=torch.float32, device=x.device)
        gemm_nt16(gh3, shadow(w2), M, C, 4 * C, EPI_NONE, out32=gh2, b_rmajor=True)
        weight_grad16(gh3, h2, grad_of(w2).view(4 * C, C))
        return _convblock_tail(ctx, x, h1, mean, rstd, gh2, go)

    @staticmethod
    def _backward_fused(ctx, go):
        x, h1, mean, rstd, h2 = ctx.saved_tensors
        w1, b1, gamma, beta, w2, b2, w3, b3 = ctx.params
        B, H, W, C = x.shape
        M = B * H * W
        go = go.contiguous()
        dev = x.device
        w2_16, w3_16 = shadow(w2), shadow(w3)
        gh2 = torch.empty((M, C), dtype=torch.float32, device=dev)
        go16 = torch.empty((M, C), dtype=torch.bfloat16, device=dev)
        h4 = torch.empty((M, 4 * C), dtype=torch.bfloat16, device=dev)
        gh3 = torch.empty((M, 4 * C), dtype=torch.bfloat16, device=dev)
        w3t, w2t = _transposed16_cached(w3, w3_16), _transposed16_cached(w2, w2_16)
        args = (go.data_ptr(), h2.data_ptr(), w2_16.data_ptr(), b2.data_ptr(), w3t.data_ptr(), w2t.data_ptr(),
                gh2.data_ptr(), go16.data_ptr(), h4.data_ptr(), gh3.data_ptr(), M, C)
        _gemm_call(4.0 * M * 4 * C * C, "sei_mlp_fused_bwd", *args)       # booked as the two data-gradient GEMMs it replaces
        if _wgrad.DWSTREAM and N.lib().sei_dwstream_bf16_eligible(C, 4 * C, C, 4 * C, M, 0):
            # the bias gradients = column sums of go16 / gh3 ride in the streamed weight-gradient launch
            weight_grad16(go16, h4, grad_of(w3).view(C, 4 * C), bias=grad_of(b3))
            weight_grad16(gh3, h2, grad_of(w2).view(4 * C, C), bias=grad_of(b2))
        else:                                           # ragged pixel counts: the column-sum kernels (go in float32)
            colsum_into(grad_of(b3), go.view(M, C))
            colsum16_into(grad_of(b2), gh3)
            weight_grad16(go16, h4, grad_of(w3).view(C, 4 * C))
            weight_grad16(gh3, h2, grad_of(w2).view(4 * C, C))
        return _convblock_tail(ctx, x, h1, mean, rstd, gh2, go)

    @staticmethod
    def joint_ctx(c1, c2, rec):
        if c1.fused != c2.fused or c1.twice != c2.twice:
            raise _NotJoint()
        return JointCtx(c1, [rec.joint(a, b) for a, b in zip(c1.saved_tensors, c2.saved_tensors)])

    @staticmethod
    def walk(ctx, g, skips):
        return ConvBlockFn16.backward(ctx, g)[0]


class DownsampleFn16(torch.autograd.Function):
    """DownsampleFn (resampler before the convolution) with the three GEMMs on bf16 operands."""

    @staticmethod
    def forward(ctx, x, gamma, beta, w, b, rate, with_skip=False):
        ctx.dtype = get_compute_dtype()
        ctx.set_materialize_grads(False)
        x = _nhwc(x)
        h, mean, rstd = layer_norm(x.view(-1, x.shape[-1]), gamma, beta)
        B, H, W, C, Co, fwd, bwd, Ho, Wo = _resample_prologue("down", x, w, rate)
        u = sepmap2_16(h.view(B, H, W, C), fwd, Ho, Wo, out16=True)
        Mo = B * Ho * Wo
        s = _mats.constant_response("down", H, W, rate, x.device, B)
        u16 = u.view(Mo, C) if u.dtype == torch.bfloat16 else cast16(u.view(Mo, C))     # (straight from the resampler where it can)
        out = _alloc((Mo, Co), torch.float32, x.device)
        gemm_nt16(u16, shadow(w), Mo, Co, C, EPI_BIAS_ROWSCALE, out32=out, bias=b, R1=s)
        ctx.save_for_backward(x, mean, rstd, u16, s)
        ctx.params, ctx.mats_t, ctx.hw = (gamma, beta, w, b), bwd, (H, W, Ho, Wo)
        ctx.with_skip, ctx.rate = with_skip, rate
        _tape(DownsampleFn16, ctx)
        out = out.view(B, Ho, Wo, Co)
        return (out, x) if with_skip else out

    @_in_forward_mode
    def backward(ctx, go, gskip=None):
        x, mean, rstd, u16, s = ctx.saved_tensors
        gamma, beta, w, b = ctx.params
        Mo, (Co, C) = x.shape[0] * ctx.hw[2] * ctx.hw[3], w.shape[:2]
        go2 = go.contiguous().view(Mo, Co)
        go16 = cast16(go2, colsum_into_=grad_of(b), row_weight=s)           # (the bias gradient from the cast's own pass)
        gu = torch.empty((Mo, C), dtype=torch.float32, device=x.device)
        gemm_nt16(go16, shadow(w), Mo, C, Co, EPI_NONE, out32=gu, b_rmajor=True)
        weight_grad16(go16, u16, grad_of(w).view(Co, C))           # after the data gradient: see ConvBlockFn16.backward
        return _downsample_tail(ctx, gu, gskip, sepmap2_16)

    @staticmethod
    def joint_ctx(c1, c2, rec):
        (x1, *mid1, _), (x2, *mid2, _) = c1.saved_tensors, c2.saved_tensors
        x = rec.joint(x1, x2)
        s = _mats.constant_response("down", c1.hw[0], c1.hw[1], c1.rate, x.device, x.shape[0])
        return JointCtx(c1, [x] + [rec.joint(a, b) for a, b in zip(mid1, mid2)] + [s])

    @staticmethod
    def walk(ctx, g, skips):
        """The gradient of the skip this layer handed on was pushed by the Upsample that received it."""
        gskip = skips.pop() if ctx.with_skip and skips else None
        return DownsampleFn16.backward(ctx, g, gskip)[0]


class UpsampleFn16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, skip, gamma, beta, w, b, rate):
        ctx.dtype = get_compute_dtype()
        x = _nhwc(x)
        B, H, W, C, Co, fwd, bwd, Ho, Wo = _resample_prologue("up", x, w, rate)
        u = sepmap2_16(x, fwd, Ho, Wo)
        M = B * Ho * Wo
        h, mean, rstd = layer_norm16(u.view(M, C), gamma, beta)
        w16 = shadow(w)
        out = _alloc((M, Co), torch.float32, x.device)
        _tape(UpsampleFn16, ctx)
        if skip is not None:
            gemm_nt16(h, w16, M, Co, C, EPI_BIAS_RES, out32=out, bias=b, R1=_check_skip(skip, (B, Ho, Wo, Co)))
        else:
            gemm_nt16(h, w16, M, Co, C, EPI_BIAS, out32=out, bias=b)
        ctx.save_for_backward(u, mean, rstd, h)
        ctx.params, ctx.mats_t, ctx.in_hw = (gamma, beta, w, b), bwd, (H, W)
        return out.view(B, Ho, Wo, Co)

    @_in_forward_mode
    def backward(ctx, go):
        u, mean, rstd, h = ctx.saved_tensors
        gamma, beta, w, b = ctx.params
        B, Ho, Wo, C = u.shape
        M, Co = B * Ho * Wo, w.shape[0]
        go = go.contiguous()
        go2 = go.view(M, Co)
        go16 = cast16(go2, colsum_into_=grad_of(b))
        gh = torch.empty((M, C), dtype=torch.float32, device=u.device)
        gemm_nt16(go16, shadow(w), M, C, Co, EPI_NONE, out32=gh, b_rmajor=True)
        weight_grad16(go16, h, grad_of(w).view(Co, C))             # after the data gradient: see ConvBlockFn16.backward
        return _upsample_tail(ctx, go, gh, sepmap2_16)

    @staticmethod
    def joint_ctx(c1, c2, rec):
        return JointCtx(c1, [rec.joint(a, b) for a, b in zip(c1.saved_tensors, c2.saved_tensors)])

    @staticmethod
    def walk(ctx, g, skips):
        """The skip's gradient waits on the stack for the Downsample that handed the skip on."""
        gx, gskip = UpsampleFn16.backward(ctx, g)[:2]
        skips.append(gskip)
        return gx


# ---------------------------------------------------------------------------------------------
# 3x3 convolutions at the ends of the U-Net                 (reference convolutional.py:174-176)
# ---------------------------------------------------------------------------------------------
class Conv3x3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, res, nchw_in, nchw_out):
        N.check_tensor(x, "conv3x3 input")
        Co, Ci = w.shape[0], w.shape[1]
        if nchw_in:
            B, _, H, W = x.shape
        else:
            B, H, W, _ = x.shape
        y = _alloc((B, Co, H, W) if nchw_out else (B, H, W, Co), torch.float32, x.device)
        _tape(Conv3x3Fn, ctx)
        if res is not None:
            N.check_tensor(res, "conv3x3 residual")
            if res.shape != y.shape:
                raise ValueError("conv3x3: residual shape mismatch")
        N.call("sei_conv3x3_fwd", x.data_ptr(), w.data_ptr(), b.data_ptr(), N.ptr(res), y.data_ptr(), B, H, W,
               Ci, Co, int(nchw_in), int(nchw_out), 0)
        ctx.save_for_backward(x)
        ctx.params, ctx.cfg = (w, b), (B, H, W, Ci, Co, nchw_in, nchw_out)
        return y

    @staticmethod
    def backward(ctx, go):
        (x,) = ctx.saved_tensors
        w, b = ctx.params
        B, H, W, Ci, Co, nchw_in, nchw_out = ctx.cfg
        go = go.contiguous()
        parts = N.lib().sei_conv3x3_bwd_weight_parts_count(B, H, W, Ci, Co, int(nchw_in), int(nchw_out)) if x.is_cuda else 0
        ncol = Co * Ci * 9 + Co
        work = torch.empty(parts * ncol, dtype=torch.float32, device=x.device) if parts else None
        if parts and defer_fold(grad_of(w), grad_of(b), None, ncol, Co * Ci * 9, N.FOLD_SPLIT, work, 0, parts):
            # the end convolutions on the matrix cores, per-workgroup sums folded with the pass's other partial sums
            N.call("sei_conv3x3_bwd_weight_parts", x.data_ptr(), go.data_ptr(), work.data_ptr(), B, H, W, Ci, Co,
                   int(nchw_in), int(nchw_out))
        else:
            N.call("sei_conv3x3_bwd_weight", x.data_ptr(), go.data_ptr(), grad_of(w).data_ptr(),
                   grad_of(b).data_ptr(), B, H, W, Ci, Co, int(nchw_in), int(nchw_out))
        gx = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            N.call("sei_conv3x3_fwd", go.data_ptr(), w.data_ptr(), None, None, gx.data_ptr(), B, H, W, Co, Ci,
                   int(nchw_out), int(nchw_in), 1)
        gres = go if ctx.needs_input_grad[3] else None
        return gx, None, None, gres, None, None

    @staticmethod
    def joint_ctx(c1, c2, rec):
        return JointCtx(c1, [rec.joint(c1.saved_tensors[0], c2.saved_tensors[0])], cfg=(c1.cfg[0] + c2.cfg[0],) + c1.cfg[1:])

    @staticmethod
    def walk(ctx, g, skips):
        return Conv3x3Fn.backward(ctx, g)[0]
