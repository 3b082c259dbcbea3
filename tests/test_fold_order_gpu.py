"""Every entry point that folds partial sums into a gradient, against oracle/fold_order.py: bit for bit.

The partial sums are the ones the producing kernel itself wrote (read back from its workspace), the destinations start
from random values (so `dst + total` is pinned too), and the model is numpy float32 in the order csrc/reduce_kernels.hip
states. tests/test_fold_order.py holds the model to the exact sums."""
import numpy as np
import pytest
import torch

from oracle import fold_order as fo

pytestmark = pytest.mark.gpu


def rand(*shape):
    return torch.randn(shape, device="cuda")


def same(got, want):
    return torch.equal(got.cpu(), torch.from_numpy(np.asarray(want)).reshape(got.shape))


def group_class(groups):
    """Which turns of the slice loop a group count takes."""
    if groups < 16:
        return "empty slices"
    if 17 <= groups <= 63:
        return "tail only"
    if groups > 64 and groups % 64 != 0:
        return "main and tail"
    return "other"


@pytest.mark.parametrize("rows,C,cls,aligned", [(77, 32, "empty slices", True), (1200, 32, "tail only", True),
                                                (5000, 32, "main and tail", True), (300, 512, "main and tail", True),
                                                (9, 8192, "empty slices", False)])
def test_layernorm_parameter_gradients(rows, C, cls, aligned):
    """sei_ln_bwd; (9, 8192) is the wide two-pass shape, whose partial sums start behind 2 * rows floats of statistics."""
    import _native as N
    torch.manual_seed(rows + C)
    need = N.lib().sei_ln_bwd_workspace(rows, C)
    parts, off = N.lib().sei_ln_bwd_part_count(rows, C), N.lib().sei_ln_bwd_part_offset(rows, C)
    assert group_class(parts) == cls and ((off * 4) % 16 == 0) == aligned
    x, gy, gamma = rand(rows, C), rand(rows, C), rand(C)
    mean = x.mean(1).contiguous(); rstd = (x.var(1, unbiased=False) + 1e-6).rsqrt().contiguous()
    gx, work = torch.empty_like(x), torch.zeros(need, device="cuda")
    args = (x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gy.data_ptr(), gx.data_ptr())
    N.call("sei_ln_bwd", *args, None, None, rows, C, work.data_ptr(), need)
    part = work[off:off + parts * 2 * C].reshape(parts, 2 * C).cpu().numpy()
    gg0, gb0 = rand(C), rand(C)
    gg, gb = gg0.clone(), gb0.clone()
    N.call("sei_ln_bwd", *args, gg.data_ptr(), gb.data_ptr(), rows, C, work.data_ptr(), need)
    assert np.array_equal(work[off:off + parts * 2 * C].reshape(parts, 2 * C).cpu().numpy(), part)
    want_g, want_b, _ = fo.fold_job(fo.FOLD_SPLIT, C, [part], gg0.cpu().numpy(), gb0.cpu().numpy())
    assert same(gg, want_g) and same(gb, want_b)


@pytest.mark.parametrize("B,H,W,C,bias", [(2, 3, 3, 8, True), (3, 6, 6, 64, True), (2, 24, 24, 32, False),
                                          (1, 5, 7, 3, True)])
def test_depthwise_weight_gradients(B, H, W, C, bias):
    """sei_dwconv7_bwd_weight_ex on its whole-image, tiled and generic paths; (1, 5, 7, 3) has 150 entries, no multiple
    of 4 or 16; one case without a bias gradient."""
    import _native as N
    torch.manual_seed(B + H + C)
    need = N.lib().sei_dwconv7_bwd_weight_workspace(B, H, W, C)
    groups = need // (50 * C)
    assert groups >= 1 and need == groups * 50 * C
    x, gy = rand(B, H, W, C), rand(B, H, W, C)
    work = torch.zeros(need, device="cuda")
    N.call("sei_dwconv7_bwd_weight_ex", x.data_ptr(), gy.data_ptr(), None, None, B, H, W, C, work.data_ptr(), need, 0)
    part = work.reshape(groups, 50 * C).cpu().numpy()
    gw0, gb0 = rand(C, 49), rand(C)
    gw, gb = gw0.clone(), gb0.clone()
    N.call("sei_dwconv7_bwd_weight_ex", x.data_ptr(), gy.data_ptr(), gw.data_ptr(), gb.data_ptr() if bias else None, B, H, W,
           C, work.data_ptr(), need, 0)
    assert np.array_equal(work.reshape(groups, 50 * C).cpu().numpy(), part)
    want_w, want_b, _ = fo.fold_job(fo.FOLD_DWCONV7, C, [part], gw0.cpu().numpy(), gb0.cpu().numpy() if bias else None)
    assert same(gw, want_w)
    assert same(gb, want_b) if bias else torch.equal(gb, gb0)


@pytest.mark.parametrize("rows,groups", [(50, 13), (4100, 1024)])
def test_swin_layernorm_parameter_gradients(rows, groups):
    """sei_ln_bwd_pad, C = 180: 360 entries, a ragged last workgroup of the fold; 4100 rows fill all 1024 partial rows."""
    import _native as N
    C = 180
    torch.manual_seed(rows)
    x, gy, gamma, res = rand(rows, C), rand(rows, C), rand(C), rand(rows, C)
    mean = x.mean(1).contiguous(); rstd = (x.var(1, unbiased=False) + 1e-5).rsqrt().contiguous()
    need = N.lib().sei_swin_partials_floats(C)
    assert need == 1024 * 2 * C and groups == min((rows + 3) // 4, 1024)
    gx, work = torch.empty_like(x), torch.zeros(need, device="cuda")
    gg0, gb0 = rand(C), rand(C)
    gg, gb = gg0.clone(), gb0.clone()
    N.call("sei_ln_bwd_pad", x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gy.data_ptr(), res.data_ptr(),
           gx.data_ptr(), gg.data_ptr(), gb.data_ptr(), rows, C, C, work.data_ptr(), need)
    part = work[:groups * 2 * C].reshape(groups, 2 * C).cpu().numpy()
    assert not np.any(work[groups * 2 * C:].cpu().numpy())                     # these are all the partial rows it wrote
    want_g, want_b, _ = fo.fold_job(fo.FOLD_SPLIT, C, [part], gg0.cpu().numpy(), gb0.cpu().numpy())
    assert same(gg, want_g) and same(gb, want_b)


def test_swin_cast_column_sums():
    """sei_cast_pad_bf16 with the column sums of the scaled rows (a bias gradient): one output, ncol = split = 180."""
    import _native as N
    C, CP, rows, groups = 180, 192, 300, 75
    torch.manual_seed(rows)
    x, scale = rand(rows, C), torch.rand(rows, device="cuda")
    y = torch.empty((rows, CP), device="cuda", dtype=torch.bfloat16)
    need = N.lib().sei_swin_partials_floats(C)
    work = torch.zeros(need, device="cuda")
    cs0 = rand(C)
    cs = cs0.clone()
    N.call("sei_cast_pad_bf16", x.data_ptr(), scale.data_ptr(), y.data_ptr(), cs.data_ptr(), rows, C, CP, work.data_ptr(), need)
    part = work[:groups * C].reshape(groups, C).cpu().numpy()
    assert np.any(part[-1]) and not np.any(work[groups * C:].cpu().numpy())
    want, _, _ = fo.fold_job(fo.FOLD_SPLIT, C, [part], cs0.cpu().numpy())
    assert same(cs, want)


@pytest.mark.parametrize("M,groups,cast", [(128, 4, True), (128, 4, False), (8256, 256, True), (8256, 256, False)])
def test_layernorm_epilogue_of_the_row_gemm(M, groups, cast):
    """sei_rowgemm_lnbwd_bf16 (K = 384, C = 180; the operands of the row-GEMM LayerNorm test in test_swinir_gpu.py): three
    sums per group, the third (the column sums of the bf16 copy) kept or dropped; 8256 rows fill all 256 partial rows."""
    import _native as N
    C, CP, K = 180, 192, 384
    gen = torch.Generator(device="cuda").manual_seed(M + K + int(cast))
    a = torch.randn((M, K), device="cuda", generator=gen).bfloat16()
    w = (0.1 * torch.randn((CP, K), device="cuda", generator=gen)).bfloat16()
    w[C:] = 0
    x = torch.randn((M, C), device="cuda", generator=gen) * 2 + 0.3
    gamma = torch.randn(C, device="cuda", generator=gen)
    res = torch.randn((M, C), device="cuda", generator=gen)
    drop = (torch.rand(M, device="cuda", generator=gen) > 0.2).float() / 0.8
    mean = x.mean(1).contiguous()
    rstd = (x.var(1, unbiased=False) + 1e-5).rsqrt().contiguous()
    gx = torch.empty((M, C), device="cuda")
    y16 = torch.empty((M, CP), device="cuda", dtype=torch.bfloat16) if cast else None
    need = N.lib().sei_rowgemm_lnbwd_work_floats(C)
    assert N.lib().sei_rowgemm_lnbwd_bf16_eligible(M, K, C) == 1 and need == 256 * 3 * C and groups == min(M // 32, 256)
    work = torch.zeros(need, device="cuda")

    def run(gg, gb, cs):
        N.call("sei_rowgemm_lnbwd_bf16", a.data_ptr(), K, w.data_ptr(), K, M, K, x.data_ptr(), gamma.data_ptr(),
               mean.data_ptr(), rstd.data_ptr(), res.data_ptr(), gx.data_ptr(), C, N.ptr(gg), N.ptr(gb),
               drop.data_ptr() if cast else None, N.ptr(y16), CP, N.ptr(cs), work.data_ptr(), need)
        return work[:groups * 3 * C].reshape(groups, 3 * C).cpu().numpy()

    part = run(None, None, None)
    gg0, gb0, cs0 = rand(C), rand(C), rand(C)
    gg, gb, cs = gg0.clone(), gb0.clone(), cs0.clone()
    assert np.array_equal(run(gg, gb, cs if cast else None), part)
    want_g, want_b, want_c = fo.fold_job(fo.FOLD_SPLIT, C, [part], gg0.cpu().numpy(), gb0.cpu().numpy(),
                                         cs0.cpu().numpy() if cast else None)
    assert same(gg, want_g) and same(gb, want_b)
    assert same(cs, want_c) if cast else torch.equal(cs, cs0)


def test_fold_many_table():
    """sei_fold_many on one table: a two-segment job on the float4 schedule, a three-segment job, a job on the scalar path
    (150 entries, the depthwise mapping) and a three-output job whose third output is dropped."""
    import _native as N
    torch.manual_seed(11)
    cases = [(fo.FOLD_SPLIT, 36, 72, (37, 200), 2),           # (kind, split, ncol, groups per segment, outputs)
             (fo.FOLD_SPLIT, 64, 128, (5, 64, 129), 2),
             (fo.FOLD_DWCONV7, 3, 150, (70, 17), 2),
             (fo.FOLD_SPLIT, 20, 60, (300,), 2)]
    arr = (N.FoldJob * len(cases))()
    keep, checks = [], []
    for j, (kind, split, ncol, groups, nout) in zip(arr, cases):
        segs = [rand(g, ncol) for g in groups]
        assert all(s.data_ptr() % 16 == 0 for s in segs)
        outs0 = [rand(split, 49) if kind == fo.FOLD_DWCONV7 else rand(split)] + [rand(split) for _ in range(nout - 1)]
        outs = [o.clone() for o in outs0]
        j.a, j.b, j.c, j.ncol, j.split, j.kind, j.nseg = outs[0].data_ptr(), outs[1].data_ptr(), None, ncol, split, kind, len(segs)
        for k, s in enumerate(segs):
            j.part[k], j.groups[k] = s.data_ptr(), s.shape[0]
        keep.append(segs)
        want = fo.fold_job(kind, split, [s.cpu().numpy() for s in segs], *[o.cpu().numpy() for o in outs0])
        checks.append((outs, want))
    N.call("sei_fold_many", arr, len(cases))
    torch.cuda.synchronize()
    for outs, want in checks:
        for got, ref in zip(outs, want):
            assert same(got, ref)
