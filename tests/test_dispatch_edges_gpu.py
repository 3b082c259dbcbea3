"""GPU: the host layer that decides which kernel runs (models/_ops.py, _native.py, losses/__init__.py), at its edges.

The kernels themselves are held to float64 elsewhere; here the routing rules are: a captured split-K launch gets only a
workspace its graph owns, bf16x3 planes sliced by rows under the joint backward, operands at a storage offset off the
16-byte grid of the float4 kernels, and bf16x3 at the GEMM shapes it turns away. Every check is against float64, or bit for
bit against the same call on an aligned copy where the path is deterministic.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def relerr(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.fixture(scope="module")
def ops():
    from models import _ops
    return _ops


def gemm_launches(log):
    """(name, M) of the sei_gemm_bf16nt* launches in a _native.record_calls log."""
    out = []
    for name, args in log:
        if name in ("sei_gemm_bf16nt", "sei_gemm_bf16nt_ws", "sei_gemm_bf16nt_ex"):
            out.append((name, args[8]))
        elif name == "sei_gemm_bf16nt_colsum":
            out.append((name, args[7]))
    return out


def recorded(fn):
    """fn()'s result and the entry points it called."""
    import _native as N
    N.record_calls(True)
    try:
        result = fn()
    finally:
        log = N.record_calls(False)
    return result, log


# ------------------------------------------------------------------ A. split-K workspaces under capture
def _side_stream(ops):
    side = torch.cuda.Stream()
    ops._SPLITK_WS.pop((0, side.cuda_stream), None)       # (torch hands out pooled streams: forget an earlier user's)
    side.wait_stream(torch.cuda.current_stream())
    return side


def test_capturing_stream_gets_only_a_workspace_it_owns(ops):
    """A stream that ran eager split-K launches has a registry workspace, which the LRU or a later own_splitk_workspace on
    the same pooled handle may free: under capture it must get none. A workspace from own_splitk_workspace (kept alive by
    the graph's owner) is handed over. Host-side only: nothing is replayed."""
    gen = torch.Generator().manual_seed(11)
    M, N, K = 2304, 128, 512
    A = torch.randn((M, K), generator=gen).bfloat16().cuda()
    Bm = torch.randn((N, K), generator=gen).bfloat16().cuda()
    out = torch.empty((M, N), device="cuda")
    side = _side_stream(ops)
    with torch.cuda.stream(side):
        ops.gemm_nt16(A, Bm, M, N, K, ops.EPI_NONE, out32=out)          # eager: a registry workspace for this stream
    torch.cuda.synchronize()
    assert (0, side.cuda_stream) in ops._SPLITK_WS
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        under_capture = ops.splitk_workspace("cuda:0")
        out.zero_()
    assert under_capture == (None, 0)
    with torch.cuda.stream(side):
        ws = ops.own_splitk_workspace("cuda:0")
    owned_graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(owned_graph, stream=side):
            owned = ops.splitk_workspace("cuda:0")
            out.zero_()
    finally:
        ops.release_splitk_workspace("cuda:0", side, ws)
    assert owned == (ws.data_ptr(), ws.numel())
    assert ops._SPLITK_WS.get((0, side.cuda_stream)) is not ws
    torch.cuda.synchronize()


def test_captured_splitk_gemms_survive_workspace_eviction(ops):
    """Eager warm-up and capture on one side stream; then eager split-K launches on SPLITK_WS_STREAMS + 1 fresh streams
    (the registry evicts) and >= 256 MiB of fresh allocations holding a pattern (freed blocks are reused). Replays stay
    within 3e-6 of float64 and leave the pattern alone."""
    gen = torch.Generator().manual_seed(12)
    shapes = [(2304, 128, 512), (2304, 128, 2048)]
    ops_in = [(torch.randn((M, K), generator=gen).bfloat16(), torch.randn((N, K), generator=gen).bfloat16())
              for M, N, K in shapes]
    refs = [A.double() @ Bm.double().T for A, Bm in ops_in]
    dev_in = [(A.cuda(), Bm.cuda()) for A, Bm in ops_in]
    outs = [torch.full((M, N), 7.0, device="cuda") for M, N, K in shapes]
    side = _side_stream(ops)
    with torch.cuda.stream(side):
        for (M, N, K), (A, Bm), out in zip(shapes, dev_in, outs):
            ops.gemm_nt16(A, Bm, M, N, K, ops.EPI_NONE, out32=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        handed = ops.splitk_workspace("cuda:0")
        for (M, N, K), (A, Bm), out in zip(shapes, dev_in, outs):
            ops.gemm_nt16(A, Bm, M, N, K, ops.EPI_NONE, out32=out)
    assert handed == (None, 0)                  # (checked before any replay: a baked-in registry pointer may be freed)
    streams = [torch.cuda.Stream() for _ in range(ops.SPLITK_WS_STREAMS + 1)]
    scratch = [torch.empty((2304, 128), device="cuda") for _ in streams]
    for st, out in zip(streams, scratch):
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            ops.gemm_nt16(dev_in[1][0], dev_in[1][1], 2304, 128, 2048, ops.EPI_NONE, out32=out)
    torch.cuda.synchronize()
    assert sum(1 for k in ops._SPLITK_WS if k[0] == 0) <= ops.SPLITK_WS_STREAMS
    n = (ops.SPLITK_WS_MIB + 16) << 18                          # int32 elements: SPLITK_WS_MIB + 16 MiB
    pattern = torch.arange(n, dtype=torch.int32, device="cuda") * 7 + 3
    torch.cuda.synchronize()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for out, ref in zip(outs, refs):
            assert relerr(out, ref) < 3e-6
    assert torch.equal(pattern, torch.arange(n, dtype=torch.int32, device="cuda") * 7 + 3)
    assert relerr(scratch[0], refs[1]) < 3e-6


# ------------------------------------------------------------------ B. bf16x3 and the joint row split
EPILOGUES = ["NONE", "BIAS", "BIAS_GELU", "BIAS_RES", "MUL_DGELU", "ACCUM", "BIAS_ROWSCALE"]


def _epilogue_case(ops, kind, M, N, gen):
    """(epilogue code, gemm keyword arguments as float32 device tensors, the float64 result as a function of the float64
    product)."""
    epi = getattr(ops, "EPI_" + kind)
    bias, res = torch.randn((N,), generator=gen), torch.randn((M, N), generator=gen)
    if kind == "NONE":
        return epi, {}, lambda r: r
    if kind == "BIAS":
        return epi, {"bias": bias.cuda()}, lambda r: r + bias.double()
    if kind == "BIAS_GELU":
        return epi, {"bias": bias.cuda(), "D2": torch.empty((M, N), device="cuda")}, lambda r: r + bias.double()
    if kind == "BIAS_RES":
        res2 = torch.randn((M, N), generator=gen)
        return epi, {"bias": bias.cuda(), "R1": res.cuda(), "R2": res2.cuda()}, \
            lambda r: r + bias.double() + res.double() + res2.double()
    if kind == "MUL_DGELU":
        p64 = res.double().requires_grad_(True)
        (dg,) = torch.autograd.grad(F.gelu(p64).sum(), p64)
        return epi, {"R1": res.cuda()}, lambda r: r * dg
    if kind == "ACCUM":
        return epi, {"out": res.cuda()}, lambda r: r + res.double()
    if kind == "BIAS_ROWSCALE":
        s = torch.rand((M,), generator=gen)
        return epi, {"bias": bias.cuda(), "R1": s.cuda()}, lambda r: r + s.double()[:, None] * bias.double()
    raise ValueError(kind)


# (3456, 512, 2048) with tb = 0 is a contracting data gradient (K = 4 N, M >= 3456): deliberately NOT split, plain or
# accumulating; every other case splits each of its three products into the two calls' rows
@pytest.mark.parametrize("M,N,K,tb,kinds,split", [
    (3456, 2048, 512, 1, EPILOGUES, True), (3456, 2048, 512, 0, EPILOGUES, True),
    (864, 8192, 2048, 1, EPILOGUES, True), (864, 8192, 2048, 0, EPILOGUES, True),
    (3456, 512, 2048, 1, EPILOGUES, True), (3456, 512, 2048, 0, ["NONE", "ACCUM"], False)])
def test_bf16x3_under_the_joint_row_split(ops, M, N, K, tb, kinds, split):
    """gemm_x3 inside joint_rows(., (2B, B)): each product as two launches over the rows of the two model calls (checked
    through the call log), every epilogue _x3_ok admits, against float64 at the bf16x3 bar."""
    gen = torch.Generator().manual_seed(M + N + K + tb)
    x = torch.randn((M, K), generator=gen)
    w = 0.05 * torch.randn((N, K) if tb else (K, N), generator=gen)
    ref = x.double() @ (w.double().T if tb else w.double())
    scale = float(ref.abs().max())
    xd, wd = x.cuda(), w.cuda()
    M1 = M * 2 // 3
    tol = 1.2e-5
    prev = ops.set_compute_dtype("bf16x3")
    try:
        for kind in kinds:
            epi, kw, want = _epilogue_case(ops, kind, M, N, gen)
            with ops.joint_rows(None, (2, 1)):
                out, log = recorded(lambda: ops.gemm(xd, wd, M, N, K, 0, tb, epi, **kw))
            launches = gemm_launches(log)
            assert any(name == "sei_split_bf16x2" for name, _ in log), kind
            if split:
                assert sorted(m for _, m in launches) == sorted([M1, M - M1] * 3), (kind, launches)
            else:
                assert [m for _, m in launches] == [M] * 3, (kind, launches)
            target = want(ref)
            assert float((out.cpu().double() - target).abs().max()) < tol * scale, kind
            if kind == "BIAS_GELU":
                assert float((kw["D2"].cpu().double() - F.gelu(target)).abs().max()) < tol * scale
    finally:
        ops.set_compute_dtype(prev)


@pytest.mark.parametrize("M,N,K,brm,case", [
    (3456, 2048, 512, 0, "rows"), (864, 8192, 2048, 0, "rows"), (3456, 512, 2048, 1, "rows"),
    (3456, 2048, 512, 0, "rowscale"), (864, 8192, 2048, 0, "rowscale"),
    (3456, 2048, 512, 1, "colsum"), (864, 8192, 2048, 1, "colsum"),
    (2304, 2304, 512, 0, "bias_of_length_M")])
def test_gemm_nt16_joint_split_cuts_only_per_row_operands(ops, M, N, K, brm, case):
    """gemm_nt16 (bf16) under joint_rows against the same call without it, float64 the judge of both: an (M, N) residual
    and the output are cut with the rows, BIAS_ROWSCALE's M-vector too, colsum= sums over both halves, and a bias whose
    length merely equals M (M == N) is never cut."""
    gen = torch.Generator().manual_seed(M + N + K + brm)
    A = torch.randn((M, K), generator=gen).bfloat16()
    B = (torch.randn((K, N) if brm else (N, K), generator=gen) / K ** 0.5).bfloat16()
    ref = A.double() @ (B.double() if brm else B.double().T)
    Ad, Bd = A.cuda(), B.cuda()
    M1 = M * 2 // 3
    bias = torch.randn((N,), generator=gen)
    res = torch.randn((M, N), generator=gen)
    s = torch.rand((M,), generator=gen)
    results = {}
    for split in (False, True):
        out32 = torch.full((M, N), float("nan"), device="cuda")
        out16, colsum = None, None
        if case == "rows":
            kw = dict(epi=ops.EPI_BIAS_RES, out32=out32, bias=bias.cuda(), R1=res.cuda())
            want = ref + bias.double() + res.double()
        elif case == "rowscale":
            kw = dict(epi=ops.EPI_BIAS_ROWSCALE, out32=out32, bias=bias.cuda(), R1=s.cuda())
            want = ref + s.double()[:, None] * bias.double()
        elif case == "colsum":
            out16 = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
            colsum = torch.full((N,), 0.5, device="cuda")
            kw = dict(epi=ops.EPI_NONE, out16=out16, colsum=colsum)
            want = ref
        else:
            assert bias.numel() == M
            kw = dict(epi=ops.EPI_BIAS, out32=out32, bias=bias.cuda())
            want = ref + bias.double()
        epi = kw.pop("epi")

        def run():
            ops.gemm_nt16(Ad, Bd, M, N, K, epi, b_rmajor=bool(brm), **kw)
        if split:
            with ops.joint_rows(None, (2, 1)):
                _, log = recorded(run)
        else:
            _, log = recorded(run)
        ms = [m for _, m in gemm_launches(log)]
        assert ms == ([M1, M - M1] if split else [M]), (split, ms)
        if out16 is not None:
            assert relerr(out16, want) < 2 ** -8
            assert relerr(colsum, out16.double().sum(0) + 0.5) < 2e-6
            results[split] = out16
        else:
            assert relerr(out32, want) < 3e-6, split
            results[split] = out32
    assert relerr(results[True], results[False].double()) < (2 ** -8 if case == "colsum" else 3e-6)


def test_joint_split_refuses_an_operand_that_is_not_an_m_by_k_matrix(ops):
    """A flat operand sliced [lo:hi] moves by elements, not rows: the joint branch of gemm_nt16 refuses it (host-side,
    nothing is launched)."""
    M, N, K = 3456, 2048, 512
    A = torch.zeros((M * K,), dtype=torch.bfloat16, device="cuda")
    B = torch.zeros((N, K), dtype=torch.bfloat16, device="cuda")
    out = torch.empty((M, N), device="cuda")
    with ops.joint_rows(None, (2, 1)):
        with pytest.raises(ValueError):
            ops.gemm_nt16(A, B, M, N, K, ops.EPI_NONE, out32=out)


# ------------------------------------------------------------------ C. views at a storage offset
def at_offset(t, k, pad=64):
    """A contiguous copy of `t` that starts k floats into a fresh allocation (k * 4 bytes off the 16-byte grid for k in
    1..3), NaN in front of it and in `pad` elements behind it: any vector access stays inside the allocation, and a
    kernel that read outside the view would show NaNs."""
    base = torch.full((k + t.numel() + pad,), float("nan"), dtype=t.dtype, device="cuda")
    v = base[k:k + t.numel()].view(t.shape)
    v.copy_(t.cuda())
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * k % 16
    return v


def same(got, ref, again=None, tol=None):
    """Bit-equal to `ref`; where `again` (a second aligned run) shows the path is not run-to-run deterministic, within
    `tol` (max-norm relative) instead."""
    if again is not None and not torch.equal(ref, again):
        assert tol is not None and relerr(got, ref) < tol
    else:
        assert torch.equal(got, ref)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_native_helpers_at_a_storage_offset(k):
    import _native as N
    from losses import _stacked_probe_input
    gen = torch.Generator().manual_seed(20 + k)
    a, b = torch.randn((2, 3, 8, 8), generator=gen), torch.randn((3, 3, 8, 8), generator=gen)
    ao, bo = at_offset(a, k), at_offset(b, 4 - k)
    # copy_into: one source, two sources, and an unaligned destination
    dst = N.copy_into(torch.empty((2, 3, 8, 8), device="cuda"), ao)
    assert torch.equal(dst, a.cuda())
    dst = N.copy_into(torch.empty((5, 3, 8, 8), device="cuda"), ao, bo)
    assert torch.equal(dst, torch.cat([a, b]).cuda())
    dsto = at_offset(torch.zeros((5, 3, 8, 8)), k)
    N.copy_into(dsto, a.cuda(), b.cuda())
    assert torch.equal(dsto, torch.cat([a, b]).cuda())
    # scale_by
    g = torch.tensor(0.37, device="cuda")
    same(N.scale_by(ao, g), N.scale_by(ao.clone(), g))
    # [y, y + tau b]: y, b or both off the grid
    y, pb = torch.randn((3, 3, 8, 8), generator=gen), torch.randn((3, 3, 8, 8), generator=gen)
    want = _stacked_probe_input(y.cuda(), pb.cuda(), 0.01)
    for yy, bb in ((at_offset(y, k), pb.cuda()), (y.cuda(), at_offset(pb, k)), (at_offset(y, k), at_offset(pb, 4 - k))):
        same(_stacked_probe_input(yy, bb, 0.01), want)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("margin", [0, 6])
def test_sure_terms_at_a_storage_offset(k, margin):
    """SureGaussianLoss with y, b and A([x_net; f(y + tau b)]) at storage offsets (the fused 2B form ProposedLoss uses) and
    through its own calls (sei_axpy on the probe): the value and the gradient bit for bit as on aligned copies."""
    import physics
    from losses.sure import SureGaussianLoss
    gen = torch.Generator().manual_seed(30 + k + margin)
    B, S = 3, 24
    y, b = torch.rand((B, 3, S, S), generator=gen), torch.randn((B, 3, S, S), generator=gen)
    if margin:
        b[:, :, :margin] = 0
        b[:, :, -margin:] = 0
        b[:, :, :, :margin] = 0
        b[:, :, :, -margin:] = 0
    y12 = torch.rand((2 * B, 3, S, S), generator=gen)
    op = physics.BlurV2(kernel=physics.get_kernel("Gaussian_R2")[None, None].cuda())
    lf = SureGaussianLoss(sigma=5 / 255, margin=margin, cropped_div=True)

    def fused(yy, bb, yy12):
        t = yy12.requires_grad_(True)
        val = lf(y=yy, x_net=None, physics=op, model=None, b=bb, y12=t)
        (g,) = torch.autograd.grad(val, t)
        return val.detach(), g

    def own(yy, bb):
        w = torch.tensor(0.9, device="cuda", requires_grad=True)
        model = lambda v: w * v + 0.05 * v * v
        val = lf(y=yy, x_net=model(yy), physics=op, model=model, b=bb)
        (gw,) = torch.autograd.grad(val, w)
        return val.detach(), gw

    want, again = fused(y.cuda(), b.cuda(), y12.cuda()), fused(y.cuda(), b.cuda(), y12.cuda())
    got = fused(at_offset(y, k), at_offset(b, 4 - k), at_offset(y12, k))
    for gt, w, a in zip(got, want, again):
        same(gt, w, a, tol=1e-6)
    want, again = own(y.cuda(), b.cuda()), own(y.cuda(), b.cuda())
    got = own(at_offset(y, k), at_offset(b, k))
    for gt, w, a in zip(got, want, again):
        same(gt, w, a, tol=1e-6)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_physics_transform_and_crop_at_a_storage_offset(k):
    """Blur and x2 / x4 downsampling A, A_adjoint and the noisy forward, the padded scaling transform (forward and
    gradient) and CropPair (the view and sei_crop_window) on offset views: bit for bit as on aligned copies."""
    import physics
    import transforms
    from crop import CropPair
    gen = torch.Generator().manual_seed(40 + k)
    x = torch.rand((3, 3, 48, 48), generator=gen)
    noise = torch.randn((3, 3, 48, 48), generator=gen)
    blur = physics.BlurV2(kernel=physics.get_kernel("Gaussian_R2")[None, None].cuda())
    ops_ = [blur, physics.Downsampling(rate=2, antialias=True), physics.Downsampling(rate=4, antialias=True)]
    for op in ops_:
        xo = at_offset(x, k)
        y = op.A(xo)
        assert torch.equal(y, op.A(x.cuda()))
        yo = at_offset(y.cpu(), 4 - k)
        assert torch.equal(op.A_adjoint(yo), op.A_adjoint(y.clone()))
    noisy = physics.GaussianNoise(sigma=0.02)
    assert torch.equal(noisy(at_offset(x, k), noise=at_offset(noise, 4 - k)), noisy(x.cuda(), noise=noise.cuda()))
    # padded scaling transform, forward and gradient
    rate, center = torch.tensor([0.5, 0.75, 1.0]), torch.rand((3, 1, 1, 2), generator=gen) * 2 - 1
    ct = torch.randn((3, 3, 48, 48), generator=gen)

    def scaled(xx, rr, cc):
        xx = xx.detach().requires_grad_(True)
        out = transforms.padded_downsampling_transform(xx, rr, cc, "bicubic", "reflection", False)
        (g,) = torch.autograd.grad(out, xx, ct.cuda())
        return out.detach(), g
    want, again = scaled(x.cuda(), rate.cuda(), center.cuda()), scaled(x.cuda(), rate.cuda(), center.cuda())
    got = scaled(at_offset(x, k), at_offset(rate, k), at_offset(center, 4 - k))
    for gt, w, a in zip(got, want, again):          # (the gradient is a scatter of float atomics)
        same(gt, w, a, tol=5e-6)
    # CropPair: the crop itself, and the window write a captured step uses
    crop = CropPair("random", 24)
    torch.manual_seed(5)
    xc, yc = crop(x.cuda(), at_offset(x, k), xy_size_ratio=1)
    torch.manual_seed(5)
    xw, yw = crop(x.cuda(), x.cuda(), xy_size_ratio=1)
    assert torch.equal(yc, yw) and torch.equal(xc, xw)
    out = torch.empty((3, 3, 24, 24), device="cuda")
    for i, j in ((0, 0), (7, 13), (30, 40)):
        crop.write_y(at_offset(x, k), i, j, out)
        ref = crop.write_y(x.cuda(), i, j, torch.empty_like(out))
        assert torch.equal(out, ref), (i, j)


def _small_unet(hidden):
    import bench
    import models
    import physics
    from optim import FlatAdam
    args = bench.reference_args("cuda", hidden=hidden, scales=3)
    p = physics.get_physics(args, "cuda")
    torch.manual_seed(0)
    model = models.get_model(args, p, "cuda")
    model.to("cuda").train()
    return args, p, model, FlatAdam(model, lr=1e-4)


@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16x3"])
def test_unet_forward_backward_at_a_storage_offset(ops, mode):
    """The U-Net (h8s3, 48 x 48, B = 3) on an input view 1 and 3 floats off the grid: restored images and the whole flat
    gradient as on an aligned copy (bit for bit where two aligned runs agree bit for bit)."""
    prev = ops.set_compute_dtype(mode)
    try:
        _, _, model, opt = _small_unet(8)
        bb = model.get_backbone()
        gen = torch.Generator().manual_seed(50)
        y = torch.rand((3, 3, 48, 48), generator=gen)
        ct = torch.randn((3, 3, 48, 48), generator=gen).cuda()

        def run(yy):
            opt.zero_grad()
            out = model(yy)
            (out * ct).sum().backward()
            torch.cuda.synchronize()
            return out.detach().clone(), bb.flat_grads.clone()

        want, again = run(y.cuda()), run(y.cuda())
        for k in (1, 3):
            got = run(at_offset(y, k))
            for gt, w, a in zip(got, want, again):
                same(gt, w, a, tol=2e-2 if mode == "bf16" else 1e-5)
    finally:
        ops.set_compute_dtype(prev)


def test_unet_joint_pair_at_a_storage_offset(ops):
    """bf16 with the joint recorder armed (the step's 2B + B pair of model calls, one backward pass over both; h32s3, the
    narrowest width whose layers all have a joint form), the 2B input a view off the grid: the recorder copies it into its
    arena (convolutional.py's copy_into). Outputs and the flat gradient as with an aligned input."""
    from models import _joint
    prev = ops.set_compute_dtype("bf16")
    try:
        _, _, model, opt = _small_unet(32)
        bb = model.get_backbone()
        gen = torch.Generator().manual_seed(51)
        y, y2 = torch.rand((3, 3, 48, 48), generator=gen), torch.rand((6, 3, 48, 48), generator=gen)
        c1, c2 = torch.randn((6, 3, 48, 48), generator=gen).cuda(), torch.randn((3, 3, 48, 48), generator=gen).cuda()

        def pair(yy2):
            opt.zero_grad()
            rec = _joint.recorder_of(bb)
            rec.expect_pair()
            out1 = model(yy2)
            out2 = model(y.cuda())
            assert rec.pair.calls == 2 and not rec.pair.broken       # (both calls recorded: one joint backward pass)
            ((out1 * c1).sum() + (out2 * c2).sum()).backward()
            torch.cuda.synchronize()
            assert rec.pair.done == [True, True]
            return out1.detach().clone(), out2.detach().clone(), bb.flat_grads.clone()

        want, again = pair(y2.cuda()), pair(y2.cuda())
        for k in (1, 3):
            got = pair(at_offset(y2, k))
            for gt, w, a in zip(got, want, again):
                same(gt, w, a, tol=2e-2)
    finally:
        ops.set_compute_dtype(prev)


@pytest.mark.parametrize("k", [1, 3])
def test_proposed_loss_step_in_bf16_at_a_storage_offset(ops, k):
    """One ProposedLoss step in bf16 (fused 2B pass, joint recorder armed and recording, injected draws; h32s3) with y a
    view off the 16-byte grid: the loss and the flat gradient as with an aligned copy of y."""
    from losses import get_loss
    from losses.sure import embed_probe
    prev = ops.set_compute_dtype("bf16")
    try:
        args, p, model, opt = _small_unet(32)
        bb = model.get_backbone()
        lf = get_loss(args, p).loss
        gen = torch.Generator().manual_seed(60)
        B = 3
        y = torch.rand((B, 3, 48, 48), generator=gen)
        m = lf.sure.div_margin
        b = embed_probe(y, torch.randn((B, 3, 48 - 2 * m, 48 - 2 * m), generator=gen), m)
        draws = {"b": b.cuda(), "rate": torch.tensor([0.75, 0.5, 1.0]).cuda(),
                 "center": (torch.rand((B, 1, 1, 2), generator=gen) * 2 - 1).cuda(),
                 "noise": torch.randn((B, 3, 48, 48), generator=gen).cuda()}

        def step(yy):
            opt.zero_grad()
            loss = lf(x=None, y=yy, model=model, draws=draws)
            assert bb._sei_joint.pair.calls == 2 and not bb._sei_joint.pair.broken
            loss.backward()
            torch.cuda.synchronize()
            return loss.detach().clone(), bb.flat_grads.clone()

        want, again = step(y.cuda()), step(y.cuda())
        got = step(at_offset(y, k))
        for gt, w, a in zip(got, want, again):
            same(gt, w, a, tol=2e-2)
        assert torch.isfinite(got[1]).all()
    finally:
        ops.set_compute_dtype(prev)


# ------------------------------------------------------------------ E. bf16x3 at the shapes it turns away
@pytest.mark.parametrize("M,N,K", [(37, 29, 19), (1, 3, 3), (130, 260, 70), (300, 96, 1000), (9, 2048, 512)])
@pytest.mark.parametrize("ta,tb", [(0, 1), (0, 0), (1, 0), (1, 1)])
def test_bf16x3_mode_at_ragged_gemm_shapes(ops, M, N, K, ta, tb):
    """ops.gemm in bf16x3 mode: the layouts sei_gemm_bf16nt takes (K % 8 == 0, N % 4 == 0; M % 8 == 0 when A is
    reduction-major, N % 8 == 0 when B is) run as three bf16 products, within 1.2e-5 of float64; every other one stays on
    the float32 GEMM, within 2e-6. The route is read from the call log, so a silent change of it fails here."""
    gen = torch.Generator().manual_seed(M * 7 + N * 3 + K + 10 * ta + tb)
    A = torch.randn((K, M) if ta else (M, K), generator=gen)
    Bm = torch.randn((N, K) if tb else (K, N), generator=gen)
    ref = (A.double().T if ta else A.double()) @ (Bm.double().T if tb else Bm.double())
    x3 = K % 8 == 0 and N % 4 == 0 and not (ta and M % 8) and not (not tb and N % 8)
    prev = ops.set_compute_dtype("bf16x3")
    try:
        out, log = recorded(lambda: ops.gemm(A.cuda(), Bm.cuda(), M, N, K, ta, tb, ops.EPI_NONE))
    finally:
        ops.set_compute_dtype(prev)
    names = [name for name, _ in log]
    if x3:
        assert "sei_gemm_f32_ex" not in names and names.count("sei_split_bf16x2") == 2 and len(gemm_launches(log)) == 3, names
        assert relerr(out, ref) < 1.2e-5
    else:
        assert names == ["sei_gemm_f32_ex"], names
        assert relerr(out, ref) < 2e-6
