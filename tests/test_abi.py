"""The C-ABI library builds, loads without a GPU, and exports exactly what include/sei_hip.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sei_hip.h")


def declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#ifdef SEI_TUNING.*?#endif", "", text, flags=re.S)     # tools-only build, not the product
    decls = {}
    for m in re.finditer(r"\b(?:int|size_t)\s+(sei_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        args = [a.strip() for a in m.group(2).split(",")]
        decls[m.group(1)] = 0 if args == ["void"] else len(args)
    return decls


def test_header_declares_entry_points():
    d = declared()
    assert len(d) >= 10 and "sei_blur_sep_circ" in d and "sei_abi_version" in d


def test_library_exports_every_declared_symbol():
    import _native
    assert os.path.exists(_native.LIB_PATH), "run `python -c 'import __graft_entry__ as g; g.build()'` first"
    handle = ctypes.CDLL(_native.LIB_PATH)       # loads on a GPU-less host: no HIP call at load time
    missing = [name for name in declared() if not hasattr(handle, name)]
    assert not missing, f"declared in sei_hip.h but not exported: {missing}"
    assert handle.sei_abi_version() == _native.ABI_VERSION == 12
    buf = ctypes.create_string_buffer(16)
    assert handle.sei_build_target(buf, 16) == 0 and buf.value == b"gfx950"


def test_product_library_has_no_debug_state():
    """re-entrant, no mutable globals. Schedule overrides are per-call arguments of the _ex entry
    points; the process-wide tuning switches and hardware probes exist only in the tools build (-DSEI_TUNING)."""
    import subprocess
    import _native
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in ("sei_debug_set_nt_tile", "sei_debug_set_dw_seg", "sei_debug_tr_probe"):
        assert not hasattr(handle, name), name
    syms = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    assert "sei_gemm_bf16nt_ex" in exported
    assert not [s_ for s_ in exported if "debug" in s_ or "gemm_bf16pp" in s_], exported
    # no writable override variable of any visibility survives in the product library
    allsyms = subprocess.run(["nm", _native.LIB_PATH], capture_output=True, text=True).stdout
    writable = [ln.split()[-1] for ln in allsyms.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "bBdD"]
    assert not [w for w in writable if "force" in w or "tuning" in w or "g_dw" in w], writable


def test_python_binding_table_matches_header():
    import _native
    d = declared()
    sized = _native.SIZE_QUERIES                          # size queries: no stream argument, size_t result
    assert set(_native.SIGNATURES) | set(sized) == set(d)
    for name, nargs in d.items():
        table = sized if name in sized else _native.SIGNATURES
        assert len(table[name]) == nargs, name


def test_argument_errors_are_reported_not_launched():
    import _native
    L = _native.lib()
    # NULL pointers / bad sizes are rejected on the host before any HIP call (safe without a GPU)
    assert L.sei_blur_sep_circ(None, None, None, None, 13, 13, 1, 8, 8, 0, None) == 10001
    assert L.sei_axpy(None, None, 1.0, None, 4, None) == 10001
    assert L.sei_scale_resample_fwd(None, None, None, None, 1, 3, 8, 8, 8, 8, None) == 10001
    # ABI 12: the step prologue, the glue kernels and the split-bf16 passes refuse bad arguments on the host too
    assert L.sei_proposed_draws(1, 0, None, 2, 3, 48, 48, 6, None, 2, None, None, None, None) == 10001
    assert L.sei_proposed_draws(1, 2, 8, 2, 3, 48, 48, 6, 8, 2, 8, 8, 8, None) == 10001          # offset % 4 != 0
    assert L.sei_proposed_draws(1, 0, 8, 2, 3, 12, 12, 6, 8, 2, 8, 8, 8, None) == 10001         # margin swallows the image
    assert L.sei_proposed_draws(1, 0, 8, 4096, 3, 48, 48, 6, 8, 2, 8, 8, 8, None) == 10001      # beyond one element per thread
    assert L.sei_proposed_draws_max_numel() == 256 * 2048
    assert L.sei_crop_window(None, None, 6, 64, 64, 0, 0, 48, None) == 10001
    assert L.sei_stack_axpy(None, None, 0.01, None, 16, None) == 10001
    assert L.sei_concat2_f32(None, 16, None, 0, None, None) == 10001
    assert L.sei_scale_dev_f32(None, None, None, 16, None) == 10001
    assert L.sei_add_scalars(None, None, None, None) == 10001
    assert L.sei_split_bf16x2(None, None, 16, None) == 10001 and L.sei_split_bf16x2(16, 16, 6, None) == 10001   # n % 4
    assert L.sei_split_bf16x3(16, 16, 16, 2, None) == 10001                                     # pattern is 0 or 1
    assert L.sei_gelu_f32(None, None, 16, None) == 10001 and L.sei_mul_dgelu_f32(None, None, 16, None) == 10001


def test_product_refuses_cpu_tensors():
    """No CPU fallback: the product path fails loudly off-GPU."""
    import torch
    import _native
    import physics
    op = physics.BlurV2(kernel=physics.get_kernel("Gaussian_R2")[None, None])
    with pytest.raises(_native.NativeLibraryError):
        op.A(torch.rand(1, 3, 16, 16))


def test_gemm_plan_query_runs_without_a_gpu():
    """sei_gemm_bf16nt_plan is host arithmetic: the schedules of the timed batch's bottleneck GEMMs (B = 32: 576 / 288
    rows) and of the reference's default batch (B = 8: 144 / 72 rows), as tests/test_loss_gpu.py pins them on the GPU."""
    import _native
    BIAS_GELU, BIAS_RES, MUL_DGELU = 2, 3, 4
    assert _native.gemm_plan(0, 0, True, False, 576, 32768, 8192, BIAS_GELU) == ("pq", 288, 256, 1)
    assert _native.gemm_plan(0, 0, True, False, 288, 32768, 8192, BIAS_GELU)[:3] == ("pq", 288, 128)
    fam, bm, bn, sk = _native.gemm_plan(0, 0, True, False, 576, 8192, 32768, BIAS_RES)
    assert (fam, bm) == ("pq", 288) and sk > 1
    assert _native.gemm_plan(0, 1, False, True, 288, 32768, 8192, MUL_DGELU)[:2] == ("pq", 288)
    assert _native.gemm_plan(0, 0, True, False, 144, 32768, 8192, BIAS_GELU)[:3] == ("nt", 128, 128)
    with pytest.raises(_native.NativeLibraryError):
        _native.gemm_plan(0, 0, True, False, 0, 128, 64, 0)


GOLDEN_PLANS = os.path.join(ROOT, "tests", "golden", "g18_gemm_plans.npz")
PLAN_AXES = ("layout", "out", "M", "N", "K", "epilogue", "ws_bytes")


def gemm_plan_table(axes):
    """The raw codes of sei_gemm_bf16nt_plan (ws_bytes = 0) / sei_gemm_bf16nt_plan_ws over the full product of `axes`
    (layout: (a_rmajor, b_rmajor) pairs, out: (float32, bf16) pairs), in product order. 0 = a refused argument set."""
    import itertools
    import numpy as np
    import _native
    L = _native.lib()
    codes = []
    for (ar, br), (f32, b16), M, N, K, epi, ws in itertools.product(*(axes[k].tolist() for k in PLAN_AXES)):
        codes.append(L.sei_gemm_bf16nt_plan_ws(ar, br, f32, b16, M, N, K, epi, ws) if ws
                     else L.sei_gemm_bf16nt_plan(ar, br, f32, b16, M, N, K, epi))
    return np.array(codes, dtype=np.uint64)


def test_gemm_dispatcher_chooses_as_recorded():
    """Every schedule the bf16 GEMM dispatcher chooses (and every argument set it refuses) over 81,920 shapes, layouts,
    epilogues and workspaces, against the codes recorded before the launch arguments were gathered into builders."""
    import itertools
    import numpy as np
    with np.load(GOLDEN_PLANS) as z:
        axes = {k: z[k] for k in PLAN_AXES}
        want = z["codes"]
    got = gemm_plan_table(axes)
    assert got.shape == want.shape == (81920,)
    # (the fixture is the parent's behaviour, not a tautology: refusals, both kernel families, atomics and slabs occur)
    fam, sk = want >> np.uint64(48), want & np.uint64(0xFFFF)
    assert ((want == 0).sum(), (fam == 1).sum(), (fam == 2).sum()) == (28930, 46302, 6688)
    assert ((sk & np.uint64(0x7FFF)) > 1).sum() == 4778 and ((sk & np.uint64(0x8000)) != 0).sum() == 566
    bad = np.flatnonzero(got != want)
    if bad.size:
        case = list(itertools.product(*(axes[k].tolist() for k in PLAN_AXES)))[int(bad[0])]
        pytest.fail(f"{bad.size} plans differ; first: {dict(zip(PLAN_AXES, case))}: "
                    f"{int(got[bad[0]]):#x}, recorded {int(want[bad[0]]):#x}")


# Fake device pointers for calls that must be refused: never dereferenced, because a refused call launches nothing.
# P is 4096-byte aligned, Q breaks the 16-byte alignment (and keeps 8).
P, Q = 4096, 4104
DW2_OPERANDS = dict(A1=P, A2=P, lda=64, B1=P, B2=P, ldb=64)
DW2_SHAPE = dict(M=64, N=64, K1=32, K2=32)
DW2_BAD = [dict(A1=None), dict(B2=None), dict(M=68, lda=72), dict(N=68, ldb=72), dict(lda=68), dict(ldb=68),
           dict(lda=56), dict(ldb=56), dict(K1=36), dict(A1=Q), dict(A2=Q), dict(B1=Q), dict(B2=Q), dict(M=0), dict(K1=0)]
ROW_OPERANDS = dict(A=P, lda=192, W=P, ldw=192)
# entry point -> (an argument list that would be ACCEPTED, in the order of the C signature; the changes that must each
# turn it into a refusal). The accepted list itself is never passed.
REFUSALS = {
    "sei_gemm_bf16nt_dw2": (
        dict(DW2_OPERANDS, D32=P, **DW2_SHAPE, accumulate=0, stream=None),
        DW2_BAD + [dict(K2=0), dict(D32=None)]),
    "sei_gemm_bf16nt_dw2_ex": (
        dict(DW2_OPERANDS, D32=P, **DW2_SHAPE, accumulate=0, tile=0, stream=None),
        DW2_BAD + [dict(K2=0), dict(D32=None), dict(tile=-1)]),
    "sei_gemm_bf16nt_dw2_adam": (
        dict(DW2_OPERANDS, param=P, exp_avg=P, exp_avg_sq=P, param_bf16=P, hyper=P, **DW2_SHAPE, stream=None),
        DW2_BAD + [dict(K2=0), dict(param=None), dict(hyper=None), dict(exp_avg=Q), dict(exp_avg_sq=Q), dict(param=Q),
                   dict(param_bf16=P + 4)]),
    "sei_gemm_bf16nt_dw2_adam_ex": (
        dict(DW2_OPERANDS, param=P, exp_avg=P, exp_avg_sq=P, param_bf16=P, hyper=P, **DW2_SHAPE, tile=0, stream=None),
        DW2_BAD + [dict(K2=0), dict(param=None), dict(hyper=None), dict(exp_avg=Q), dict(exp_avg_sq=Q), dict(param=Q),
                   dict(param_bf16=P + 4), dict(tile=-1), dict(tile=2), dict(tile=15), dict(tile=31), dict(tile=32)]),
    "sei_gemm_bf16nt_dw2_bf16out": (
        dict(DW2_OPERANDS, D16=P, **DW2_SHAPE, stream=None),
        DW2_BAD + [dict(K2=0), dict(D16=None), dict(D16=P + 4)]),
    "sei_gemm_bf16nt_dw2_taps": (           # (K2 = 0 is accepted here: one segment)
        dict(DW2_OPERANDS, D32=P, **DW2_SHAPE, accumulate=0, ntaps=9, tap_rows=P, tap_ld=4096, stream=None),
        DW2_BAD + [dict(K2=-8), dict(D32=None), dict(tap_rows=None), dict(ntaps=0), dict(ntaps=10), dict(tap_ld=4095)]),
    "sei_gemm_bf16nt_conv": (
        dict(Ap=P, cin_pad=64, row_off9=P, B=P, ldb=576, D32=P, D16=None, M=128, N=64, epilogue=0, bias=None, stream=None),
        [dict(Ap=None), dict(row_off9=None), dict(B=None), dict(D32=None), dict(Ap=Q), dict(B=Q), dict(cin_pad=96, ldb=864),
         dict(cin_pad=0), dict(ldb=568), dict(ldb=580), dict(epilogue=2, bias=P), dict(epilogue=3, bias=P),
         dict(epilogue=5), dict(epilogue=1)]),
    "sei_gemm_bf16nt_conv_unpad": (
        dict(Ap=P, cin_pad=64, row_off9=P, B=P, ldb=576, y=P, res=None, Bimg=1, H=8, W=8, N=64, bias=P, act=0, stream=None),
        [dict(Ap=None), dict(y=None), dict(B=Q), dict(y=Q), dict(res=Q), dict(cin_pad=96, ldb=864), dict(ldb=568),
         dict(N=66), dict(act=2), dict(res=P, bias=None), dict(H=0)]),
    "sei_gemm_bf16nt_ws": (
        dict(A=P, lda=64, a_rmajor=0, B=P, ldb=64, b_rmajor=0, D32=P, D16=None, M=64, N=64, K=64, epilogue=0, bias=None,
             R1=None, R2=None, D2_16=None, colsum=None, ws=P, ws_bytes=1 << 20, tile=0, band=0, splitk=0, stream=None),
        [dict(ws_bytes=16383), dict(ws_bytes=0), dict(tile=-1), dict(band=-1), dict(splitk=-1), dict(A=Q), dict(K=60),
         dict(colsum=P), dict(epilogue=1)]),
    "sei_rowgemm_bf16": (                   # SEI_EPI_BIAS_RES, float32 out
        dict(ROW_OPERANDS, D32=P, ld32=192, D16=None, ld16=0, M=64, N=192, K=192, nv=192, epilogue=3, bias=P, R1=P,
             R2=None, ldr=192, stream=None),
        [dict(M=96), dict(N=200), dict(K=576), dict(lda=196), dict(ldw=196), dict(lda=184), dict(ldw=184), dict(A=Q),
         dict(W=Q), dict(A=None), dict(nv=190), dict(nv=196, ld32=196, ldr=196), dict(bias=None), dict(R1=None),
         dict(epilogue=5, R2=P, R1=None), dict(lda=1 << 25)]),
    "sei_rowgemm_lnbwd_bf16": (
        dict(ROW_OPERANDS, lda=384, ldw=384, M=64, K=384, x=P, gamma=P, mean=P, rstd=P, res=P, gx=P, C=192, ggamma=None,
             gbeta=None, row_scale=None, y16=None, ldy=0, colsum=None, work=P, work_floats=256 * 3 * 200, stream=None),
        [dict(M=96), dict(K=192), dict(lda=388), dict(lda=376), dict(ldw=376), dict(A=Q), dict(W=Q), dict(W=None),
         dict(C=190), dict(C=196), dict(x=None), dict(res=None), dict(lda=1 << 25)]),
    "sei_rowgemm_dgelu_bf16": (
        dict(ROW_OPERANDS, A2=P, lda2=192, W2=P, ldw2=192, bias2=P, nv=384, D16=P, ld16=384, M=64, N=384, K=192,
             stream=None),
        [dict(M=96), dict(N=192), dict(K=384), dict(lda=196), dict(lda=184), dict(ldw=184), dict(lda2=184), dict(A=Q),
         dict(A2=Q), dict(W2=Q), dict(A=None), dict(nv=0), dict(nv=388), dict(bias2=None), dict(lda=1 << 25),
         dict(lda2=1 << 25)]),
    "sei_rowgemm_ln_bf16": (
        dict(ROW_OPERANDS, M=64, K=192, C=180, bias=P, row_scale=None, res=P, out=P, gamma=P, beta=P, eps=1e-5,
             ones_col=0, h16=P, ldh=192, mean=P, rstd=P, stream=None),
        [dict(M=96), dict(K=576), dict(lda=196), dict(lda=184), dict(ldw=184), dict(A=Q), dict(W=Q), dict(A=None),
         dict(C=190), dict(C=192), dict(bias=None), dict(res=None), dict(lda=1 << 25)]),
    "sei_rowgemm_gelu_bf16": (
        dict(ROW_OPERANDS, bias=P, nv=384, D16=P, ld16=384, M=64, N=384, K=192, one_at=-1, stream=None),
        [dict(M=96), dict(N=192), dict(K=384), dict(lda=196), dict(lda=184), dict(ldw=184), dict(A=Q), dict(W=Q),
         dict(W=None), dict(nv=380), dict(nv=388), dict(bias=None), dict(one_at=384), dict(lda=1 << 25)]),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_gemm_entry_points_refuse_bad_arguments(name):
    """The bf16 GEMM entry points that have no plan query: each bad argument set -- a null or misaligned operand, sizes
    and strides off the 8-element grid, a stride below the row, an empty second segment, an option outside its list,
    an epilogue without its inputs -- is refused on the host (SEI_ERR_BAD_ARG), before any HIP call."""
    import _native
    fn = getattr(_native.lib(), name)
    accepted, changes = REFUSALS[name]
    assert len(accepted) == len(_native.SIGNATURES[name])
    for change in changes:
        assert set(change) <= set(accepted), change
        args = dict(accepted, **change)
        assert args != accepted
        assert fn(*args.values()) == 10001, f"{name} accepted {change}"
