"""Every kernel that inlines sei_adam_element against the float64 model of torch.optim.Adam in tests/adam_ref.py, at the
edges of its launch: adam_vec_kernel / adam_kernel (sei_adam_fused, float32 and bf16 gradients, unaligned views, ragged
tails), dip_adam_kernel (sei_dip_adam), the Adam epilogues of the 128 x 128 loop and of the quadrant schedule
(sei_gemm_bf16nt_dw2_adam_ex) and FlatAdam on the device. The bounds are adam_ref's stage-wise ones, per element:
4 u (|m| + S) for exp_avg, 8 u (b2 v + (1 - b2) S^2) for exp_avg_sq, u |p| + 8 u |delta_k| for the parameter.

Worst observed multiples on an MI355X (exp_avg in u (|m| + S), exp_avg_sq in u (b2 v + (1 - b2) S^2), the parameter in
u (|p| + |delta_k|)), per entry point:
    sei_adam_fused, float32 gradients (all sets, sizes, views)   1.21   3.97   4.69
    sei_adam_fused, bf16 gradients                                0.71   3.52   2.99
    sei_dip_adam                                                  1.03   3.96   3.95
    sei_gemm_bf16nt_dw2_adam_ex, tiles 1 / 30 / 33 / 0 alike      1.03   4.14   4.01
    FlatAdam.step (six steps)                                     1.00   4.11   3.87
against bounds of 4, 8 and (u |p| + 8 u |delta_k|); the float32 emulation on the CPU reaches 1.7, 5.2 and 4.5.

Not exercised: the grid-stride repeat of adam_vec_kernel (beyond 2^31 elements, the 2^20-workgroup cap) and the sharded
multi-GPU step.
"""
import ctypes

import numpy as np
import pytest
import torch

import adam_ref as R

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 4, 5, 7, 8, 1023, 2048, 2049, 4 * 512 * 3 + 5)
PAD = 8                                             # elements of every backing buffer around the stepped view


@pytest.fixture(scope="module")
def N():
    import _native
    return _native


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).cuda()              # a copy: the helper's arrays are read-only
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def report(entry, worst):
    print(f"ADAM-WORST {entry} m={worst.m:.3f} v={worst.v:.3f} p={worst.p:.3f}")


def fused(N, p, g, m, v, hyper, grad_scale=1.0, p16=None):
    N.call("sei_adam_fused", p.data_ptr(), g.data_ptr(), int(g.dtype == torch.bfloat16), m.data_ptr(), v.data_ptr(),
           p.numel(), *hyper[:5], hyper.step, grad_scale, N.ptr(p16))


def device_scalars(N, hyper):
    d = torch.zeros(6, device="cuda")
    N.call("sei_adam_scalars_to_device", *hyper[:5], hyper.step, d.data_ptr())
    return d


def aligned_run(N, arrays, hyper, grad_scale=1.0, g=None):
    """sei_adam_fused on fresh, 16-byte-aligned copies: (p, m, v, bf16 shadow) after the step."""
    p, g32, m, v = (dev(a) for a in arrays)
    g = g32 if g is None else g
    p16 = torch.zeros(p.numel(), device="cuda", dtype=torch.bfloat16)
    assert all(t.data_ptr() % 16 == 0 for t in (p, g, m, v, p16))
    fused(N, p, g, m, v, hyper, grad_scale, p16)
    return p, m, v, p16


# ------------------------------------------------------------------ sei_adam_fused, float32 gradients
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("hyper", R.HYPER_SETS, ids=lambda h: f"step{h.step}")
def test_fused_step_against_float64(N, hyper, grad_scale):
    """n = 100003 (25000 quads and a tail of 3): the three stage-wise bounds; the bf16 shadow is the rounded new p."""
    arrays = R.case(hyper)
    p, m, v, p16 = aligned_run(N, arrays, hyper, grad_scale)
    worst = R.check_stages(*arrays, host(p), host(m), host(v), hyper, grad_scale, what="sei_adam_fused")
    report("sei_adam_fused", worst)
    assert same_bits(p16, p.bfloat16())
    without = dev(arrays[0])                                          # and the same step without a shadow
    m2, v2 = dev(arrays[2]), dev(arrays[3])
    fused(N, without, dev(arrays[1]), m2, v2, hyper, grad_scale)
    assert same_bits(without, p) and same_bits(m2, m) and same_bits(v2, v)


def _views(arrays, offsets, g16=None):
    """Backing buffers (p, g, m, v, shadow) of n + 2 PAD elements filled with a recognisable pattern, the case's values at
    [PAD + off, PAD + off + n) of each: the buffers, the views and copies of the buffers as they were."""
    n = arrays[0].size
    rng = np.random.default_rng(7)
    backs, views = [], []
    for k, off in enumerate(offsets):
        if k == 4:
            back = dev(rng.uniform(1.0, 2.0, n + 2 * PAD).astype(np.float32), torch.bfloat16)
        elif k == 1 and g16 is not None:
            back = dev(rng.uniform(1.0, 2.0, n + 2 * PAD).astype(np.float32), torch.bfloat16)
            back[PAD + off:PAD + off + n] = g16
        else:
            back = dev(rng.uniform(1.0, 2.0, n + 2 * PAD).astype(np.float32))
            back[PAD + off:PAD + off + n] = dev(arrays[k])
        assert back.data_ptr() % 16 == 0
        backs.append(back)
        views.append(back[PAD + off:PAD + off + n])
    return backs, views, [b.clone() for b in backs]


def _outside_untouched(backs, before, offsets, n, what):
    for k, (b, b0, off) in enumerate(zip(backs, before, offsets)):
        lo, hi = PAD + off, PAD + off + n
        assert same_bits(b[:lo], b0[:lo]) and same_bits(b[hi:], b0[hi:]), f"{what}: buffer {k} changed outside its view"
    assert same_bits(backs[1], before[1]), f"{what}: the gradient was written"


@pytest.mark.parametrize("n", SIZES)
def test_fused_step_on_views_of_one_buffer(N, n):
    """Every size crossed with an element offset 0 .. 3 of all five views (non-zero: the scalar kernel; the tail takes it
    in any case), and grad / shadow / exp_avg_sq misaligned alone: p, m, v and the shadow bit-identical to the aligned
    launch on a copy ("identical per-element arithmetic"), inside the bounds, and nothing outside [off, off + n) of the
    four written buffers changes (FlatAdam.step steps sub-ranges of one bucket)."""
    hyper, grad_scale = R.HYPER_SETS[1], 0.125
    arrays = R.case(hyper, n)
    want = aligned_run(N, arrays, hyper, grad_scale)
    report("sei_adam_fused", R.check_stages(*arrays, *(host(t) for t in want[:3]), hyper, grad_scale, what=f"aligned n={n}"))
    assert same_bits(want[3], want[0].bfloat16())
    layouts = [(k,) * 5 for k in range(4)] + [(0, 1, 0, 0, 0), (0, 0, 0, 0, 1), (0, 0, 0, 3, 0)]
    for offsets in layouts:
        backs, (p, g, m, v, p16), before = _views(arrays, offsets)
        fused(N, p, g, m, v, hyper, grad_scale, p16)
        torch.cuda.synchronize()
        for name, got, ref in zip(("p", "exp_avg", "exp_avg_sq", "shadow"), (p, m, v, p16), want):
            assert same_bits(got, ref), f"n={n} offsets={offsets}: {name} differs from the aligned launch"
        _outside_untouched(backs, before, offsets, n, f"n={n} offsets={offsets}")


# ------------------------------------------------------------------ bf16 gradients
@pytest.mark.parametrize("n", SIZES)
def test_fused_step_with_bf16_gradients(N, n):
    """grad_is_bf16 with the gradient 0, 2, 4, 6 bytes past an 8-byte boundary (0: grad_quad's 8-byte loads, else the
    scalar decode). Element i carries bf16(i), so a swapped pair of a quad shows. Inside the bounds against the model fed
    the rounded gradient; bit-identical to the float32 launch on the widened gradient."""
    hyper = R.HYPER_SETS[1]
    p0, _, m0, v0 = R.case(hyper, n)
    g16 = torch.arange(n, dtype=torch.float32).bfloat16().cuda()
    wide = g16.float()
    arrays = (p0, host(wide), m0, v0)
    assert n < 4 or len(set(arrays[1][:4].tolist())) == 4
    want = aligned_run(N, arrays, hyper)
    report("sei_adam_fused[bf16 grad]", R.check_stages(*arrays, *(host(t) for t in want[:3]), hyper, what=f"widened n={n}"))
    for off in range(4):
        offsets = (0, off, 0, 0, 0)
        backs, (p, g, m, v, p16), before = _views(arrays, offsets, g16=g16)
        assert g.dtype == torch.bfloat16 and g.data_ptr() % 8 == 2 * off
        fused(N, p, g, m, v, hyper, 1.0, p16)
        torch.cuda.synchronize()
        for name, got, ref in zip(("p", "exp_avg", "exp_avg_sq", "shadow"), (p, m, v, p16), want):
            assert same_bits(got, ref), f"n={n}, gradient {2 * off} bytes off: {name} differs from the float32 launch"
        _outside_untouched(backs, before, offsets, n, f"bf16 n={n} off={off}")


# ------------------------------------------------------------------ special values
SPECIAL = R.Hyper(1e-3, 0.9, 0.999, 1e-8, 0.0, 3)


def _kernel_runs(N):
    """name -> run(p, g, m, v, hyper) -> (p, m, v) as numpy, one per element-wise kernel (the vector kernel on aligned
    quads, the scalar kernel through a view one element off, sei_dip_adam with its scalars on the device)."""
    def vec(p, g, m, v, hyper):
        assert p.size % 4 == 0
        return tuple(host(t) for t in aligned_run(N, (p, g, m, v), hyper)[:3])

    def scalar(p, g, m, v, hyper):
        _, (pp, gg, mm, vv, _), _ = _views((p, g, m, v), (1,) * 5)
        fused(N, pp, gg, mm, vv, hyper)
        return host(pp), host(mm), host(vv)

    def dip(p, g, m, v, hyper):
        pp, gg, mm, vv = (dev(a) for a in (p, g, m, v))
        N.call("sei_dip_adam", pp.data_ptr(), gg.data_ptr(), mm.data_ptr(), vv.data_ptr(), p.size,
               device_scalars(N, hyper).data_ptr())
        return host(pp), host(mm), host(vv)

    return {"adam_vec_kernel": vec, "adam_kernel": scalar, "dip_adam_kernel": dip}


@pytest.mark.parametrize("kernel", ["adam_vec_kernel", "adam_kernel", "dip_adam_kernel"])
def test_special_values(N, kernel):
    """One table per element-wise kernel: against the model where it is finite, by class otherwise (zero gradient and
    moments, exp_avg_sq overflowing, g^2 underflowing, one NaN and one inf gradient among finite ones)."""
    run = _kernel_runs(N)[kernel]
    f = np.float32
    p0 = R.state(16, seed=3)[0]
    zeros = np.zeros(16, f)
    # g = m = v = 0: without weight decay nothing moves; with it, the model
    pk, mk, vk = run(p0, zeros, zeros, zeros, SPECIAL)
    assert pk.tobytes() == p0.tobytes() and not mk.any() and not vk.any()
    decayed = SPECIAL._replace(weight_decay=0.1)
    pk, mk, vk = run(p0, zeros, zeros, zeros, decayed)
    R.check_stages(p0, zeros, zeros, zeros, pk, mk, vk, decayed, what=f"{kernel}, zero gradient with weight decay")
    assert np.all(pk != p0)
    # g = +-3e38: exp_avg_sq overflows, the update vanishes
    _, _, m0, v0 = R.state(16, seed=4)
    big = np.where(np.arange(16) % 2, f(3e38), f(-3e38)).astype(f)
    pk, mk, vk = run(p0, big, m0, v0, SPECIAL)
    assert np.all(np.isposinf(vk)) and np.all(np.isfinite(mk)) and np.all(np.isfinite(pk))
    assert np.all(np.abs(pk.astype(np.float64) - p0) <= R.U * np.abs(p0))
    m1 = R.adam_step64(p0, big, m0, v0, **SPECIAL._asdict())[1]
    assert np.all(np.abs(mk - m1) <= R.BOUND_M * R.U * R.scales(p0, big, m0, v0, SPECIAL)[0])
    # |g| = 1e-25: g^2 underflows in float32, eps alone is the denominator
    tiny = np.where(np.arange(16) % 2, f(1e-25), f(-1e-25)).astype(f)
    pk, mk, vk = run(p0, tiny, zeros, zeros, SPECIAL)
    assert np.all(np.isfinite(pk)) and np.all(np.isfinite(mk)) and not vk.any()
    h = R.rounded(SPECIAL)
    limit = h.lr / (1.0 - h.beta1 ** h.step) * np.abs(mk.astype(np.float64)) / h.eps
    assert np.all(np.abs(pk.astype(np.float64) - p0) <= limit)
    m1 = R.adam_step64(p0, tiny, zeros, zeros, **SPECIAL._asdict())[1]
    assert np.all(mk != 0) and np.all(np.abs(mk - m1) <= R.BOUND_M * R.U * np.abs(tiny.astype(np.float64)))
    # one NaN and one inf gradient among finite ones: theirs alone
    _, g0, m0, v0 = R.state(16, seed=5)
    bad = g0.copy()
    bad[2], bad[9] = np.nan, np.inf
    clean = run(p0, g0, m0, v0, SPECIAL)
    pk, mk, vk = run(p0, bad, m0, v0, SPECIAL)
    assert np.isnan(pk[2]) and np.isnan(pk[9])
    others = np.ones(16, bool)
    others[[2, 9]] = False
    for got, ref in zip((pk, mk, vk), clean):
        assert got[others].tobytes() == ref[others].tobytes()
    R.check_stages(*(a[others] for a in (p0, g0, m0, v0, pk, mk, vk)), SPECIAL, what=f"{kernel}, beside NaN and inf")


# ------------------------------------------------------------------ the step's six scalars
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.95, 0.9999)])
def test_adam_scalars(N, betas):
    """out6[4] = lr / (1 - b1^t) and out6[5] = 1 / sqrt(1 - b2^t) within one float32 ulp of the float64 values rounded to
    float32; out6[0 .. 3] the inputs' bits; the device array the host array bit for bit."""
    lr, eps, wd = 3e-4, 1e-8, 0.01
    for step in (1, 2, 10, 1000, 10 ** 6):
        hyper = R.Hyper(lr, *betas, eps, wd, step)
        out = (ctypes.c_float * 6)()
        N.call("sei_adam_scalars", *hyper[:5], step, ctypes.cast(out, ctypes.c_void_p))
        got = np.array(list(out), dtype=np.float32)
        h = R.rounded(hyper)
        assert got[:4].tobytes() == np.array([h.beta1, h.beta2, h.eps, h.weight_decay], np.float32).tobytes()
        want = np.array([h.lr / (1.0 - h.beta1 ** step), 1.0 / np.sqrt(1.0 - h.beta2 ** step)]).astype(np.float32)
        ulps = np.abs(got[4:].view(np.int32).astype(np.int64) - want.view(np.int32))
        assert ulps.max() <= 1, (step, got[4:], want)
        assert host(device_scalars(N, hyper)).tobytes() == got.tobytes()


# ------------------------------------------------------------------ sei_dip_adam
@pytest.mark.parametrize("hyper", [R.HYPER_SETS[1], R.HYPER_SETS[4]], ids=lambda h: f"step{h.step}")
@pytest.mark.parametrize("n", [1, 255, 256, 257, R.N_MAIN])
def test_dip_adam(N, n, hyper):
    """Scalars through sei_adam_scalars_to_device: inside the bounds, and the bits of sei_adam_fused at grad_scale 1."""
    arrays = R.case(hyper, n)
    p, g, m, v = (dev(a) for a in arrays)
    N.call("sei_dip_adam", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, device_scalars(N, hyper).data_ptr())
    report("sei_dip_adam", R.check_stages(*arrays, host(p), host(m), host(v), hyper, what="sei_dip_adam"))
    assert same_bits(g, dev(arrays[1]))
    for got, ref in zip((p, m, v), aligned_run(N, arrays, hyper)):
        assert same_bits(got, ref)


# ------------------------------------------------------------------ the two GEMM epilogues
def _exact_operands(M, Nn, K1, K2, seed):
    """bf16 operands whose two-segment product A1^T B1 + A2^T B2 is exact in float32 in any order of the additions:
    integers in [-2, 2], A's times a power of two in [2^-12, 2^4] per row of the product; |sum| <= 4 (K1 + K2) < 2^24 in
    units of the row's scale. Returns the device operands and the float64 gradient."""
    rng = np.random.default_rng(seed)
    scale = 2.0 ** rng.integers(-12, 5, M)
    As = [rng.integers(-2, 3, (k, M)).astype(np.float64) * scale for k in (K1, K2)]
    Bs = [rng.integers(-2, 3, (k, Nn)).astype(np.float64) for k in (K1, K2)]
    grad = As[0].T @ Bs[0] + As[1].T @ Bs[1]
    ops = [dev(a.astype(np.float32), torch.bfloat16) for a in As + Bs]
    assert all(np.array_equal(host(o.double()), a) for o, a in zip(ops, As + Bs))
    assert np.array_equal(grad.astype(np.float32).astype(np.float64), grad)
    return ops, grad


@pytest.mark.parametrize("hyper", [R.HYPER_SETS[1], R.HYPER_SETS[3]], ids=lambda h: f"step{h.step}")
@pytest.mark.parametrize("M,Nn,K1,K2", [(256, 256, 64, 64), (512, 768, 96, 200), (136, 520, 96, 200)])
def test_gemm_epilogues_against_float64(N, M, Nn, K1, K2, hyper):
    """sei_gemm_bf16nt_dw2_adam_ex on an exactly representable gradient (a whole 256 x 256 tile; K tails in both segments;
    ragged edges; no claim about which kernel a tile code ends on): the float64 product is what every accumulator holds, so
    the stage-wise bounds apply unchanged, all tile codes agree bit for bit, and with sei_gemm_bf16nt_dw2 followed by
    sei_adam_fused -- also where that storing GEMM splits K."""
    (A1, A2, B1, B2), grad = _exact_operands(M, Nn, K1, K2, seed=M + K2)
    p0, _, m0, v0 = R.state(M * Nn, seed=1)
    arrays = (p0, grad.reshape(-1), m0, v0)
    assert R.informative_fraction(*arrays, hyper) >= R.MIN_INFORMATIVE
    scalars = device_scalars(N, hyper)
    out = {}
    for tile in (1, 30, 33, 0):
        p, m, v = (dev(a).view(M, Nn) for a in (p0, m0, v0))
        sh = torch.zeros((M, Nn), device="cuda", dtype=torch.bfloat16)
        N.call("sei_gemm_bf16nt_dw2_adam_ex", A1.data_ptr(), A2.data_ptr(), M, B1.data_ptr(), B2.data_ptr(), Nn,
               p.data_ptr(), m.data_ptr(), v.data_ptr(), sh.data_ptr(), scalars.data_ptr(), M, Nn, K1, K2, tile)
        worst = R.check_stages(*arrays, *(host(t).reshape(-1) for t in (p, m, v)), hyper, what=f"tile {tile}")
        report(f"sei_gemm_bf16nt_dw2_adam_ex[tile {tile}]", worst)
        assert same_bits(sh, p.bfloat16()), f"tile {tile}: the shadow is not the rounded new parameter"
        out[tile] = (p, m, v, sh)
    for tile in (30, 33, 0):
        for name, a, b in zip(("p", "exp_avg", "exp_avg_sq", "shadow"), out[tile], out[1]):
            assert same_bits(a, b), f"tile {tile} against the loop: {name}"
    stored = torch.empty((M, Nn), device="cuda")
    N.call("sei_gemm_bf16nt_dw2", A1.data_ptr(), A2.data_ptr(), M, B1.data_ptr(), B2.data_ptr(), Nn, stored.data_ptr(),
           M, Nn, K1, K2, 0)
    assert np.array_equal(host(stored).astype(np.float64), grad)
    separate = aligned_run(N, arrays, hyper, g=stored.view(-1))
    for name, a, b in zip(("p", "exp_avg", "exp_avg_sq", "shadow"), separate, out[1]):
        assert same_bits(a, b.view(-1)), f"GEMM then sei_adam_fused against the epilogue: {name}"


@pytest.mark.parametrize("tile", [1, 30, 33])
def test_gemm_epilogue_special_values(N, tile):
    """The special-value table of the element-wise kernels through the epilogues: a rank-one gradient a_r b_c (one
    non-zero reduction row; b_c = +-1) gives every row of the 256 x 256 weight one class -- a_r = 0, 1.75 * 2^127 (the
    bf16 next to 3e38), 2^-83 (1.03e-25), NaN, inf or an ordinary value."""
    M = Nn = 256
    K1 = K2 = 64
    f = np.float32
    rng = np.random.default_rng(11)
    rows = np.arange(M) % 8
    zero, big, tiny, nan_row, inf_row = (rows == k for k in (0, 1, 2, 4, 5))
    a = np.choose(rows, [0.0, 1.75 * 2.0 ** 127, 2.0 ** -83, 1.0, 1.0, 2.0, 0.5, 3.0])
    a_bad = np.where(nan_row, np.nan, np.where(inf_row, np.inf, a))
    b = np.where(np.arange(Nn) % 2, -1.0, 1.0)
    B1 = rng.integers(-2, 3, (K1, Nn)).astype(np.float64)
    B1[0] = b
    B2 = rng.integers(-2, 3, (K2, Nn)).astype(np.float64)
    p0, _, m0, v0 = (x.reshape(M, Nn).copy() for x in R.state(M * Nn, seed=6))
    m0[zero | tiny], v0[zero | tiny] = 0, 0

    def run(a_row, hyper):
        A1 = np.zeros((K1, M))
        A1[0] = a_row
        ops = [dev(x.astype(f), torch.bfloat16) for x in (A1, np.zeros((K2, M)), B1, B2)]
        assert np.array_equal(host(ops[0][0].double()), a_row, equal_nan=True)
        p, m, v = dev(p0), dev(m0), dev(v0)
        sh = torch.zeros((M, Nn), device="cuda", dtype=torch.bfloat16)
        N.call("sei_gemm_bf16nt_dw2_adam_ex", ops[0].data_ptr(), ops[1].data_ptr(), M, ops[2].data_ptr(), ops[3].data_ptr(), Nn,
               p.data_ptr(), m.data_ptr(), v.data_ptr(), sh.data_ptr(), device_scalars(N, hyper).data_ptr(), M, Nn, K1, K2, tile)
        assert same_bits(sh, p.bfloat16())
        return host(p), host(m), host(v)

    grad = a[:, None] * b[None, :]
    for hyper in (SPECIAL, SPECIAL._replace(weight_decay=0.1)):
        pk, mk, vk = run(a, hyper)
        # the model applies where float32 exp_avg_sq neither overflows nor (bare 1e-25 gradients) underflows
        finite = ~big if hyper.weight_decay else ~(big | tiny)
        R.check_stages(*(x[finite].reshape(-1) for x in (p0, grad, m0, v0, pk, mk, vk)), hyper, what=f"tile {tile}, finite rows")
        sm = R.scales(p0, grad, m0, v0, hyper)[0]
        m1 = R.adam_step64(p0, grad, m0, v0, **hyper._asdict())[1]
        assert np.all(np.abs(mk - m1) <= R.BOUND_M * R.U * sm)
        # exp_avg_sq overflows: the update vanishes
        assert np.all(np.isposinf(vk[big])) and np.all(np.isfinite(mk)) and np.all(np.isfinite(pk))
        assert np.all(np.abs(pk[big].astype(np.float64) - p0[big]) <= R.U * np.abs(p0[big]))
        if hyper.weight_decay == 0:
            # nothing to do: nothing moves
            assert pk[zero].tobytes() == p0[zero].tobytes() and not mk[zero].any() and not vk[zero].any()
            # g^2 underflows in float32: eps alone is the denominator
            h = R.rounded(hyper)
            limit = h.lr / (1.0 - h.beta1 ** h.step) * np.abs(mk[tiny].astype(np.float64)) / h.eps
            assert not vk[tiny].any() and np.all(mk[tiny] != 0)
            assert np.all(np.abs(pk[tiny].astype(np.float64) - p0[tiny]) <= limit)
        else:
            assert np.all(pk[zero] != p0[zero])
        # NaN and inf gradients are their rows' alone
        pb, mb, vb = run(a_bad, hyper)
        bad = nan_row | inf_row
        assert np.all(np.isnan(pb[bad]))
        for got, ref in zip((pb, mb, vb), (pk, mk, vk)):
            assert got[~bad].tobytes() == ref[~bad].tobytes()


# ------------------------------------------------------------------ FlatAdam on the device
def test_flat_adam_on_the_device(N):
    """Six steps of FlatAdam over the small U-Net's bucket (hidden 8, scales 3) with fresh gradients in flat_grads, lr
    changed before step 3, the state through torch.optim.Adam and into a new FlatAdam before step 5: every step inside
    the stage-wise bounds against one model step from the device state before it (re-anchored, so the bounds stay
    single-step while step, lr and the bias corrections advance); the bf16 copy follows; the per-parameter state_dict
    is the flat moments."""
    from models.convolutional import ConvolutionalModel
    from optim import FlatAdam
    torch.manual_seed(0)
    model = ConvolutionalModel(in_channels=3, upsampling_rate=2, residual=True, inner_residual=True, num_conv_blocks=1,
                               hidden_channels=8, inout_convs=True, scales=3).cuda()
    model.compute_dtype = "bf16"                        # the step then writes the bf16 copy of the bucket too
    betas, eps, wd = (0.8, 0.95), 1e-6, 1e-2
    opt = FlatAdam(model, lr=3e-4, betas=betas, eps=eps, weight_decay=wd)
    flat, grads = model.flat_params, model.flat_grads
    n = flat.numel()
    lr = 3e-4
    for step in range(1, 7):
        if step == 3:
            lr = 1e-4
            opt.param_groups[0]["lr"] = lr
        if step == 5:
            through = torch.optim.Adam(model.parameters(), lr=1.0)
            through.load_state_dict(opt.state_dict())
            opt = FlatAdam(model, lr=1.0)
            opt.load_state_dict(through.state_dict())
            group = opt.param_groups[0]
            assert (group["lr"], tuple(group["betas"]), group["eps"], group["weight_decay"]) == (lr, betas, eps, wd)
        st = opt.state[flat]
        assert st["step"] == step - 1
        g = R.state(n, seed=20 + step)[1]
        grads.copy_(dev(g))
        before = (host(flat), g, host(st["exp_avg"]), host(st["exp_avg_sq"]))
        opt.step()
        hyper = R.Hyper(lr, *betas, eps, wd, step)
        worst = R.check_stages(*before, host(flat), host(st["exp_avg"]), host(st["exp_avg_sq"]), hyper,
                               what=f"FlatAdam step {step}")
        report("FlatAdam.step", worst)
        assert same_bits(model.flat_shadow, flat.bfloat16())
        assert R.informative_fraction(*before, hyper) >= R.MIN_INFORMATIVE
    st = opt.state[flat]
    assert st["step"] == 6
    saved = opt.state_dict()["state"]
    params = list(model.parameters())
    assert sorted(saved) == list(range(len(params)))
    for i, prm in enumerate(params):
        off = (prm.data_ptr() - flat.data_ptr()) // 4
        assert float(saved[i]["step"]) == 6.0
        for key in ("exp_avg", "exp_avg_sq"):
            assert same_bits(saved[i][key], st[key][off:off + prm.numel()].view(prm.shape))
