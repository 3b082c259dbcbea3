"""The 128 x 256 tile of the weight-gradient GEMM with the Adam epilogue (sei_gemm_bf16nt_dw2_adam_ex, tile 16: 32-row
stages on a three-stage ring) against the 128 x 128 loop (tile 1) and against sei_adam_fused on the gradient that
sei_gemm_bf16nt_dw2 stores: parameter, exp_avg, exp_avg_sq and the bf16 shadow BIT FOR BIT, after two consecutive steps
from non-zero moments, with and without weight decay. The wide tile issues the same 32x32x16 MFMA steps in the same k
order as the loop (its 32-row stage is half a 64-row k-tile; rows past K are zero and add nothing), so nothing may differ.

Shapes: one tile with a full and a half k-tile per segment; a k-tile that straddles the segment boundary at a 32-row
stage; the benchmark's K over several tiles; a segment boundary INSIDE a 32-row stage with a ragged K tail (the wide
tile's own general staging path); and shapes the wide tile cannot take, which the automatic entry must leave on 128 x 128.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

WIDE, LOOP, AUTO = 16, 1, 0
LR, BETA1, BETA2, EPS = 2e-4, 0.9, 0.99, 1e-8


@pytest.fixture(scope="module")
def N():
    import _native
    return _native


def operands(M, Nn, K1, K2, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    A1, A2 = ((0.05 * torch.randn((k, M), device="cuda", generator=gen)).bfloat16() for k in (K1, K2))
    B1, B2 = (torch.randn((k, Nn), device="cuda", generator=gen).bfloat16() for k in (K1, K2))
    p0 = 0.02 * torch.randn((M, Nn), device="cuda", generator=gen)
    m0 = 1e-3 * torch.randn((M, Nn), device="cuda", generator=gen)
    v0 = 1e-5 * torch.rand((M, Nn), device="cuda", generator=gen) + 1e-7
    return (A1, A2, B1, B2), (p0, m0, v0)


def fresh(state):
    p0, m0, v0 = state
    return [p0.clone(), m0.clone(), v0.clone(), torch.zeros(p0.shape, device="cuda", dtype=torch.bfloat16)]


def hyper_of(N, wd, step):
    host = (ctypes.c_float * 6)()
    N.call("sei_adam_scalars", LR, BETA1, BETA2, EPS, wd, step, ctypes.cast(host, ctypes.c_void_p))
    return torch.tensor(list(host), device="cuda")


def gemm_step(N, ops, st, hyper, tile):
    A1, A2, B1, B2 = ops
    (K1, M), (K2, Nn) = A1.shape, B2.shape
    N.call("sei_gemm_bf16nt_dw2_adam_ex", A1.data_ptr(), A2.data_ptr(), M, B1.data_ptr(), B2.data_ptr(), Nn, st[0].data_ptr(),
           st[1].data_ptr(), st[2].data_ptr(), st[3].data_ptr(), hyper.data_ptr(), M, Nn, K1, K2, tile)


def separate_step(N, ops, st, wd, step):
    """the stored gradient (128 x 128 tiles, K not split at these sizes: see the plan assertion) and then sei_adam_fused"""
    A1, A2, B1, B2 = ops
    (K1, M), (K2, Nn) = A1.shape, B2.shape
    grad = torch.empty((M, Nn), device="cuda")
    N.call("sei_gemm_bf16nt_dw2", A1.data_ptr(), A2.data_ptr(), M, B1.data_ptr(), B2.data_ptr(), Nn, grad.data_ptr(), M, Nn,
           K1, K2, 0)
    N.call("sei_adam_fused", st[0].data_ptr(), grad.data_ptr(), 0, st[1].data_ptr(), st[2].data_ptr(), M * Nn, LR, BETA1,
           BETA2, EPS, wd, step, 1.0, st[3].data_ptr())


def two_steps(N, ops, state, wd, tile):
    st = fresh(state)
    for step in (5, 6):
        if tile is None:
            separate_step(N, ops, st, wd, step)
        else:
            gemm_step(N, ops, st, hyper_of(N, wd, step), tile)
    torch.cuda.synchronize()
    return st


def assert_same(got, want, what):
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "shadow"), got, want):
        assert torch.equal(a, b), (what, name, int((a != b).sum()))


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("M,Nn,K1,K2", [(128, 256, 64, 32), (256, 512, 96, 160), (384, 768, 576, 288), (256, 512, 104, 96)])
def test_wide_tile_equals_the_loop_and_the_separate_adam_step(N, M, Nn, K1, K2, wd):
    assert N.adam_gemm_plan(M, Nn, K1, K2, WIDE) == ("nt", 128, 256, 1)
    assert N.adam_gemm_plan(M, Nn, K1, K2, LOOP) == ("nt", 128, 128, 1)
    assert N.gemm_plan(1, 1, True, False, M, Nn, K1 + K2, 0)[3] == 1          # the stored gradient does not split K
    ops, state = operands(M, Nn, K1, K2, seed=M + K1)
    wide = two_steps(N, ops, state, wd, WIDE)
    assert float((wide[0] - state[0]).abs().max()) > 1e-5                       # the steps moved the parameter
    assert_same(wide, two_steps(N, ops, state, wd, LOOP), "wide tile vs 128 x 128 loop")
    assert_same(wide, two_steps(N, ops, state, wd, None), "wide tile vs sei_adam_fused on the stored gradient")


@pytest.mark.parametrize("M,Nn", [(256, 384), (136, 512)])
def test_shapes_the_wide_tile_cannot_take_stay_on_the_loop(N, M, Nn):
    """N % 256 != 0 / M % 128 != 0: the automatic entry (and a forced wide tile) plans 128 x 128 tiles and still matches the
    forced loop and the separate step bit for bit (ragged rows included: at K = 256 the stored gradient does not split K)."""
    K1, K2 = 96, 160
    for tile in (AUTO, WIDE):
        assert N.adam_gemm_plan(M, Nn, K1, K2, tile) == ("nt", 128, 128, 1)
    assert N.gemm_plan(1, 1, True, False, M, Nn, K1 + K2, 0)[3] == 1
    ops, state = operands(M, Nn, K1, K2, seed=M + Nn)
    auto = two_steps(N, ops, state, 0.01, AUTO)
    assert_same(auto, two_steps(N, ops, state, 0.01, LOOP), "automatic entry vs 128 x 128 loop")
    assert_same(auto, two_steps(N, ops, state, 0.01, WIDE), "automatic entry vs a wide tile that falls back")
    assert_same(auto, two_steps(N, ops, state, 0.01, None), "automatic entry vs sei_adam_fused on the stored gradient")


def test_the_step_s_shapes_take_the_wide_tile_automatically(N):
    """host arithmetic: whole tiles that fill both workgroup slots of all 256 CUs in every round, and a reduction of at
    least 2048 or at least eight rounds (one round of a short reduction measured slower than the loop)"""
    for M, Nn, K1, K2 in ((2048, 8192, 2304, 1152), (8192, 2048, 2304, 1152), (8192, 32768, 576, 288), (32768, 8192, 576, 288)):
        assert N.adam_gemm_plan(M, Nn, K1, K2, AUTO) == ("nt", 128, 256, 1)
    assert N.adam_gemm_plan(8192, 2048, 576, 288, AUTO) == ("nt", 128, 128, 1)           # 512 tiles, K = 864
    assert N.adam_gemm_plan(2048, 6144, 640, 1032, AUTO) == ("nt", 128, 128, 1)          # 384 wide tiles: three quarters of a round
    assert N.adam_gemm_plan(2048, 8192 + 256, 640, 1032, AUTO) == ("nt", 128, 128, 1)    # 528 tiles: 16 in a second round


def test_wide_tile_replayed_from_a_graph_equals_eager_calls(N):
    M, Nn, K1, K2 = 256, 512, 96, 160
    ops, state = operands(M, Nn, K1, K2, seed=9)
    hyper = hyper_of(N, 0.01, 5)
    eager = fresh(state)
    for _ in range(2):
        gemm_step(N, ops, eager, hyper, WIDE)
    st = fresh(state)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            gemm_step(N, ops, st, hyper, WIDE)
    for t, t0 in zip(st, fresh(state)):             # whatever the capture did to the state, start from the same values
        t.copy_(t0)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert_same(st, eager, "two replays vs two eager calls")
