"""GEMM dispatch of the layer functions: compute-dtype scopes, the float32 / bf16 / bf16x3 GEMM entry points, the
split-K workspace registry, and the joint row split of one backward pass over the step's two model calls.

Everything here is pointers + sizes; shapes are checked on the host. models/_wgrad.py (the weight-gradient scheduler)
and models/_ops.py (the layer functions) build on it.
"""
import os

import torch

import _native as N
from ._shadow import split_x2

EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_MUL_DGELU, EPI_ACCUM, EPI_BIAS_ROWSCALE = range(7)

_GEMM_PROFILE = None     # bench.py: list of (flops, entry point, ctypes args) recorded while enabled
# "bf16x3": the float32 layer functions with every GEMM evaluated as three bf16 MFMA products (gemm_x3 below)
_GEMM_ENTRY = {"f32": "sei_gemm_f32_ex", "bf16": "sei_gemm_bf16_ex", "bf16x3": None}
_COMPUTE_DTYPE = "f32"
_DTYPE_SCOPE = []            # innermost compute_dtype_scope (a model call or a backward function of one) wins


def set_compute_dtype(name):
    """The PROCESS DEFAULT of the arithmetic type of the 1x1-convolution GEMMs: "f32" (exact-f32 MFMA; the parity mode),
    "bf16" (bf16 MFMA with f32 accumulation; GEMM-only activations stored in bf16) or "bf16x3" (float32 storage and layer
    functions as "f32"; each GEMM as three bf16 MFMA products of bf16 head / remainder operands, f32 accumulation: 16
    mantissa bits per operand, the second parity mode). Everything else is f32 either way. A backbone
    may carry its own (`backbone.compute_dtype = "f32" | "bf16"`, None = the default): its forward pass and the backward
    functions it recorded run under it (`compute_dtype_scope`), so two models of different modes can live in one process."""
    global _COMPUTE_DTYPE
    if name not in _GEMM_ENTRY:
        raise ValueError(f"compute dtype must be one of {sorted(_GEMM_ENTRY)}, got {name!r}")
    previous, _COMPUTE_DTYPE = _COMPUTE_DTYPE, name
    return previous


def get_compute_dtype(owner=None):
    """The mode in effect: `owner`'s own (a backbone), else the innermost scope's, else the process default."""
    own = getattr(owner, "compute_dtype", None) if owner is not None else None
    if own is not None:
        return own
    return _DTYPE_SCOPE[-1] if _DTYPE_SCOPE else _COMPUTE_DTYPE


class compute_dtype_scope:
    """`with compute_dtype_scope(backbone_or_name):` -- the GEMMs issued inside use that backbone's mode (or the named
    one); a backbone without its own mode, or None, leaves the mode in effect unchanged."""

    def __init__(self, owner_or_name):
        name = owner_or_name if isinstance(owner_or_name, str) or owner_or_name is None \
            else getattr(owner_or_name, "compute_dtype", None)
        if name is not None and name not in _GEMM_ENTRY:
            raise ValueError(f"compute dtype must be one of {sorted(_GEMM_ENTRY)}, got {name!r}")
        self.name = name

    def __enter__(self):
        if self.name is not None:
            _DTYPE_SCOPE.append(self.name)
        return self

    def __exit__(self, *exc):
        if self.name is not None:
            _DTYPE_SCOPE.pop()
        return False


def _in_forward_mode(fn):
    """Decorator for the backward of an autograd Function whose forward stored `ctx.dtype = get_compute_dtype()`."""
    def backward(ctx, *grads):
        with compute_dtype_scope(getattr(ctx, "dtype", None)):
            return fn(ctx, *grads)
    return staticmethod(backward)


def profile_gemms(enable):
    """Record every GEMM launch (entry point + arguments + algorithmic FLOPs) while enabled, so that
    bench.py can re-issue exactly those launches back to back between HIP events (roofline leg)."""
    global _GEMM_PROFILE
    records, _GEMM_PROFILE = _GEMM_PROFILE, ([] if enable else None)
    return records


def _gemm_call(flops, entry, *args):
    if _GEMM_PROFILE is not None:
        _GEMM_PROFILE.append((flops, entry, args))
    N.call(entry, *args)


def gemm(A, Bm, M, Nn, K, ta, tb, epi, out=None, bias=None, R1=None, R2=None, D2=None, allow_splitk=True):
    if out is None:
        out = torch.empty((M, Nn), dtype=torch.float32, device=A.device)
    if get_compute_dtype() == "bf16x3" and _x3_ok(A, Bm, M, Nn, K, ta, tb, epi, out, R1, D2):
        return gemm_x3(A, Bm, M, Nn, K, ta, tb, epi, out, bias, R1, R2, D2)
    _gemm_call(2.0 * M * Nn * K, _GEMM_ENTRY[get_compute_dtype()] or "sei_gemm_f32_ex", A.data_ptr(), Bm.data_ptr(), out.data_ptr(), M, Nn, K,
               ta, tb, epi, N.ptr(bias), N.ptr(R1), N.ptr(R2), N.ptr(D2), 1, 0, 0, 0, int(allow_splitk))
    return out


# Split-K workspace of the quadrant GEMM (sei_gemm_bf16nt_ws, include/sei_hip.h): tile counters in its first 16 KiB (zero
# between launches: every launch leaves them zero) + the slabs the K slices meet in. The ticket protocol indexes counters
# and slabs by tile ordinal alone, so two launches in flight at once must never share one: a workspace belongs to ONE
# (device, stream) -- launches on a stream are a chain. Eager launches find theirs in a small registry (created on the
# stream's first eager use; the least recently used one is dropped when a device has SPLITK_WS_STREAMS of them). A stream
# that is CAPTURING gets none unless it OWNS one (the graph bakes the pointer in, and a registry workspace may be dropped by
# the LRU or replaced by own_splitk_workspace on the same pooled stream handle while the graph lives; replays would then
# write slabs and tickets into freed memory): those launches take the float-atomics path (sei_gemm_bf16nt / _colsum).
# graphs.GraphedLossStep therefore warms up and captures on one side stream with a workspace OF ITS OWN
# (`own_splitk_workspace` ... `release_splitk_workspace`: registered for that stream while the step is being built, kept
# alive by the graph's owner afterwards): its replays -- serialised by the graph itself -- never share it with anybody,
# whatever stream they are launched from, and torch handing the same pooled stream to somebody else later cannot alias it.
# SEI_SPLITK_WS_MIB = 0 switches the workspace off everywhere (round-1..5 path).
SPLITK_WS_MIB = int(os.environ.get("SEI_SPLITK_WS_MIB", "256"))
SPLITK_WS_STREAMS = 4
SPLITK_COUNTER_BYTES = 16 << 10
_SPLITK_WS = {}              # (device index, stream handle) -> uint8 tensor; insertion order = least recently used first


def _splitk_key(device):
    dev = torch.device(device).index
    if dev is None:
        dev = torch.cuda.current_device()
    return dev, torch.cuda.current_stream(dev).cuda_stream


def splitk_workspace(device):
    """(pointer, bytes) of the split-K workspace of (`device`, its current stream), or (None, 0): switched off, or the
    stream is capturing without a workspace of its own (own_splitk_workspace)."""
    if SPLITK_WS_MIB <= 0:
        return None, 0
    key = _splitk_key(device)
    if torch.cuda.is_current_stream_capturing() and not getattr(_SPLITK_WS.get(key), "_sei_owned", False):
        return None, 0
    ws = _SPLITK_WS.pop(key, None)
    if ws is None:
        mine = [k for k in _SPLITK_WS if k[0] == key[0]]
        if len(mine) >= SPLITK_WS_STREAMS:
            del _SPLITK_WS[mine[0]]              # (freed in stream order by the caching allocator: its launches are queued)
        ws = torch.zeros(SPLITK_WS_MIB << 20, dtype=torch.uint8, device=f"cuda:{key[0]}")
    _SPLITK_WS[key] = ws                         # most recently used last
    return ws.data_ptr(), ws.numel()


def own_splitk_workspace(device):
    """A NEW workspace registered for (`device`, its current stream), returned to the caller, who keeps it alive for as
    long as launches recorded on this stream may run (a captured graph) and calls release_splitk_workspace when it has
    finished recording. None when switched off."""
    if SPLITK_WS_MIB <= 0:
        return None
    key = _splitk_key(device)
    ws = _SPLITK_WS[key] = torch.zeros(SPLITK_WS_MIB << 20, dtype=torch.uint8, device=f"cuda:{key[0]}")
    ws._sei_owned = True                         # (the only kind splitk_workspace hands to a capturing stream)
    return ws


def release_splitk_workspace(device, stream, ws):
    """Take `ws` (from own_splitk_workspace on `stream`) out of the registry: later eager launches on that stream handle
    get a workspace of their own."""
    dev = torch.device(device).index
    if dev is None:
        dev = torch.cuda.current_device()
    key = (dev, stream.cuda_stream)
    if ws is not None and _SPLITK_WS.get(key) is ws:
        del _SPLITK_WS[key]


def reset_splitk_counters(device):
    """Zero the tile counters of every workspace of `device`, each on the stream that owns it (a launch that never
    finished -- a fault survived by the process -- would leave tickets behind, and no slice would ever draw the last one).
    Not under capture. graphs.GraphedLossStep calls it before its warm-up."""
    dev = torch.device(device).index
    if dev is None:
        dev = torch.cuda.current_device()
    for (d, handle), ws in _SPLITK_WS.items():
        if d == dev:
            with torch.cuda.stream(torch.cuda.ExternalStream(handle, device=f"cuda:{dev}") if handle else
                                   torch.cuda.default_stream(dev)):
                ws[:SPLITK_COUNTER_BYTES].zero_()


def gemm_nt16(A16, B16, M, Nn, K, epi, out32=None, out16=None, bias=None, R1=None, R2=None, D2_16=None,
              lda=None, ldb=None, a_rmajor=False, b_rmajor=False, tile=0, band=0, flops=None, _whole=False, colsum=None):
    """D[M,N] = op(A16) op(B16) on the direct-to-LDS bf16 kernel. A16 is (M,K) [or (K,M) when a_rmajor],
    B16 is (N,K) [or (K,N) when b_rmajor]; K % 8 == 0. Outputs as given. tile / band: an explicit schedule
    choice (sei_gemm_bf16nt_ex; tests and tools), 0 = the library's dispatch. flops: the algorithmic FLOP count
    to book for the roofline leg when the operands are zero-padded (default 2 M N K). colsum (float32, (N,)): += the column
    sums of the bf16 result out16 (sei_gemm_bf16nt_colsum: a bias gradient riding in the data gradient's epilogue)."""
    # (the CONTRACTING data gradients gh2 = gh3 W2 -- float32 out, K = 4 N, split K -- run faster on the joint rows: their
    # K splits fill the rounds whatever the row count. tools/exp_joint_rows.py, merged vs the two launches: 3456 x 2048 x 8192
    # 153 vs 104 + 71 us, 864 x 8192 x 32768 479 vs 310 + 187, 13824 x 512 x 2048 44 vs 37 + 30; the expanding ones with
    # GELU' lose merged: 3456 x 8192 x 2048 147 vs 85 + 51, 864 x 32768 x 8192 492 vs 287 + 169.)
    contracting = (out32 is not None and out16 is None and epi in (EPI_NONE, EPI_ACCUM) and b_rmajor and K == 4 * Nn
                   and (M >= 3456 or K >= 8192))               # (also 864 x 2048 x 8192: 61 vs 53 + 39, exp_joint_rows2.py)
    if _JOINT_SPLIT is not None and not _whole and not a_rmajor and max(Nn, K) >= 2048 and not (tile or band) and lda is None \
            and not contracting:
        # One backward pass over the rows of both model calls (models/_joint.py) -- but the deep levels' GEMMs are tuned to
        # the row counts of the separate calls (2304 / 1152 and 576 / 288 rows are whole rounds of 288-row tiles on 256 CUs;
        # 3456 and 864 rows are 1.5 rounds: measured 168 us against 79 + 58): their rows go as the two launches they were
        B1, B2 = _JOINT_SPLIT
        M1 = M * B1 // (B1 + B2)
        if 0 < M1 < M and M1 % 8 == 0 and (M - M1) % 8 == 0:
            if A16.dim() != 2 or A16.shape[0] != M:      # (rows are sliced below: a flat or reshaped operand would move by
                raise ValueError(                      # elements, not rows -- gemm_x3 hands its planes over as (M, K))
                    f"gemm_nt16 under joint_rows: A16 must be an (M, K) matrix with M = {M}, got {tuple(A16.shape)}")
            # an epilogue operand is cut with the rows when it is per-row data: an (M, Nn) matrix in any view with M * Nn
            # elements, or BIAS_ROWSCALE's M-vector -- never by a leading dimension that happens to equal M
            def cut(t, lo, hi):
                if t is None:
                    return None
                if t.dim() == 1 and t.numel() == M:
                    return t[lo:hi]
                if t.numel() == M * Nn:
                    return t.reshape(M, Nn)[lo:hi]
                return t
            for lo, hi in ((0, M1), (M1, M)):
                gemm_nt16(A16[lo:hi], B16, hi - lo, Nn, K, epi, out32=cut(out32, lo, hi), out16=cut(out16, lo, hi), bias=bias,
                          R1=cut(R1, lo, hi), R2=cut(R2, lo, hi), D2_16=cut(D2_16, lo, hi),
                          ldb=ldb, b_rmajor=b_rmajor, flops=None if flops is None else flops * (hi - lo) / M, _whole=True,
                          colsum=colsum)
            return
    if lda is None:
        lda = M if a_rmajor else K
    if ldb is None:
        ldb = Nn if b_rmajor else K
    args = (A16.data_ptr(), lda, int(a_rmajor), B16.data_ptr(), ldb, int(b_rmajor), N.ptr(out32), N.ptr(out16), M, Nn,
            K, epi, N.ptr(bias), N.ptr(R1), N.ptr(R2), N.ptr(D2_16))
    fl = 2.0 * M * Nn * K if flops is None else float(flops)
    ws, ws_bytes = (None, 0) if (tile or band or a_rmajor) else splitk_workspace(A16.device)
    if colsum is not None:
        if out32 is not None or out16 is None or epi not in (EPI_NONE, EPI_MUL_DGELU) or tile or band or bias is not None \
                or R2 is not None or D2_16 is not None:
            raise ValueError("gemm_nt16(colsum=): a bf16 result with EPI_NONE / EPI_MUL_DGELU on the automatic dispatch")
        if ws is not None:
            _gemm_call(fl, "sei_gemm_bf16nt_ws", *args, colsum.data_ptr(), ws, ws_bytes, 0, 0, 0)
            return
        _gemm_call(fl, "sei_gemm_bf16nt_colsum", A16.data_ptr(), lda, int(a_rmajor), B16.data_ptr(), ldb, int(b_rmajor),
                   out16.data_ptr(), M, Nn, K, epi, N.ptr(R1), colsum.data_ptr())
        return
    if tile or band:
        _gemm_call(fl, "sei_gemm_bf16nt_ex", *args, int(tile), int(band))
    elif ws is not None:
        # (K slices of the quadrant kernel meet in slabs of the workspace: no zero fill, no float atomics)
        _gemm_call(fl, "sei_gemm_bf16nt_ws", *args, None, ws, ws_bytes, 0, 0, 0)
    else:
        _gemm_call(fl, "sei_gemm_bf16nt", *args)


_JOINT_SPLIT = None      # (B1, B2) while one backward pass serves the step's two model calls (joint_rows), else None


class joint_rows:
    """`with joint_rows(backbone, (B1, B2)):` -- one backward pass over the rows of the step's two model calls
    (models/_joint.py): gemm_nt16 and _wgrad.weight_grad16 split their operands' rows B1 : B2 into the two calls' segments
    (None: a single call walked alone, nothing to split). One pass runs at a time, so the split is process-wide; `backbone`
    says whose pass it is."""

    def __init__(self, backbone, batches):
        self.batches = batches

    def __enter__(self):
        global _JOINT_SPLIT
        self.prev, _JOINT_SPLIT = _JOINT_SPLIT, self.batches
        return self

    def __exit__(self, *exc):
        global _JOINT_SPLIT
        _JOINT_SPLIT = self.prev
        return False


# ---------------------------------------------------------------------------------------------
# --compute_dtype bf16x3: a float32 GEMM as three bf16 MFMA products (csrc/bf16x3.hip has the arithmetic and the error
# bound). Operands are split once into bf16 head / remainder PLANES ((2, rows, cols): either plane is a dense operand of
# sei_gemm_bf16nt in whatever orientation the float32 GEMM read the tensor), weights once per optimizer step. The three
# launches accumulate into the float32 result, small terms first; additive epilogues (bias, residuals, the running
# gradient) ride on the first launch, GELU / GELU' follow as element-wise passes.
# ---------------------------------------------------------------------------------------------
def _x3_ok(A, Bm, M, Nn, K, ta, tb, epi, out=None, R1=None, D2=None):
    """Shapes sei_gemm_bf16nt takes (K % 8, 16-byte rows of the reduction-major operands) and operands the float4 passes
    around it take (sei_split_bf16x2 / x3 read A and Bm, sei_gelu_f32 / sei_mul_dgelu_f32 out with D2 / R1: 16-byte
    aligned); anything else -- the 3-channel ends of the network never come here -- stays on the float32 GEMM."""
    if not (A.is_cuda and A.dtype == torch.float32 and Bm.dtype == torch.float32 and K % 8 == 0 and Nn % 4 == 0):
        return False
    if (ta and M % 8) or (not tb and Nn % 8) or A.numel() % 4 or Bm.numel() % 4 or not A.is_contiguous() \
            or not Bm.is_contiguous():
        return False
    if not N.aligned(A, Bm, out, R1 if epi == EPI_MUL_DGELU else None, D2 if epi == EPI_BIAS_GELU else None):
        return False
    return epi in (EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_MUL_DGELU, EPI_ACCUM, EPI_BIAS_ROWSCALE)


def gemm_x3(A, Bm, M, Nn, K, ta, tb, epi, out, bias=None, R1=None, R2=None, D2=None):
    """gemm()'s contract (float32 operands as stored: A (M, K) or (K, M) when ta, Bm (N, K) when tb else (K, N))."""
    arm, brm = bool(ta), not tb
    if arm and brm and epi == EPI_ACCUM:
        # a weight gradient (both operands reduction-major, a large output that is read-modify-written): the three
        # products in ONE launch whose reduction runs over the stacked planes, K' = 3 K
        a3 = torch.empty((3 * K, M), dtype=torch.bfloat16, device=A.device)
        b3 = torch.empty((3 * K, Nn), dtype=torch.bfloat16, device=A.device)
        N.call("sei_split_bf16x3", A.data_ptr(), a3.data_ptr(), A.numel(), 0)
        N.call("sei_split_bf16x3", Bm.data_ptr(), b3.data_ptr(), Bm.numel(), 1)
        gemm_nt16(a3, b3, M, Nn, 3 * K, EPI_ACCUM, out32=out, a_rmajor=True, b_rmajor=True, flops=2.0 * M * Nn * K)
        return out
    # each plane as the 2-D matrix gemm_nt16 reads ((K, M) / (K, N) when reduction-major): under joint_rows it slices A's
    # planes by rows
    a2 = split_x2(A).view(2, -1)[:, :M * K].unflatten(1, (K, M) if arm else (M, K))
    b2 = split_x2(Bm).view(2, -1)[:, :Nn * K].unflatten(1, (K, Nn) if brm else (Nn, K))
    (a_hi, a_lo), (b_hi, b_lo) = a2, b2
    third = 2.0 * M * Nn * K / 3.0                    # (algorithmic FLOPs are booked once over the three launches)
    first = {EPI_BIAS_GELU: EPI_BIAS, EPI_MUL_DGELU: EPI_NONE}.get(epi, epi)
    gemm_nt16(a_lo, b_hi, M, Nn, K, first, out32=out, bias=bias, R1=R1 if first != EPI_NONE else None,
              R2=R2 if first == EPI_BIAS_RES else None, a_rmajor=arm, b_rmajor=brm, flops=third)
    gemm_nt16(a_hi, b_lo, M, Nn, K, EPI_ACCUM, out32=out, a_rmajor=arm, b_rmajor=brm, flops=third)
    gemm_nt16(a_hi, b_hi, M, Nn, K, EPI_ACCUM, out32=out, a_rmajor=arm, b_rmajor=brm, flops=third)
    if epi == EPI_BIAS_GELU:
        N.call("sei_gelu_f32", out.data_ptr(), D2.data_ptr(), out.numel())
    elif epi == EPI_MUL_DGELU:
        N.call("sei_mul_dgelu_f32", out.data_ptr(), R1.data_ptr(), out.numel())
    return out


def gemm_mixed(A, Bm, M, Nn, K, ta, tb, epi, out=None, bias=None, R1=None, R2=None, D2=None, allow_splitk=True):
    """Register-staged bf16-MFMA GEMM; each operand may be stored as float32 or bfloat16."""
    if out is None:
        out = torch.empty((M, Nn), dtype=torch.float32, device=A.device)
    _gemm_call(2.0 * M * Nn * K, "sei_gemm_bf16_mixed", A.data_ptr(), int(A.dtype == torch.bfloat16), Bm.data_ptr(),
               int(Bm.dtype == torch.bfloat16), out.data_ptr(), M, Nn, K, ta, tb, epi, N.ptr(bias), N.ptr(R1),
               N.ptr(R2), N.ptr(D2), 1, 0, 0, 0, int(allow_splitk))
    return out
