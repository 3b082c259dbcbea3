"""sei_gemm_bf16nt_dw2_adam_group: several weight-gradient GEMMs with the Adam epilogue as ONE launch of the 128 x 256 tile,
against every job alone through sei_gemm_bf16nt_dw2_adam_ex on the same tile (16) and on the 128 x 128 loop (1):
parameter, exp_avg, exp_avg_sq and the bf16 copy BIT FOR BIT after two steps from non-zero moments, with and without
weight decay. A job's tiles run the kernel body of tile 16 -- the same MFMA steps in the same order, the same Adam
arithmetic -- so nothing may differ; what the grouped launch adds is the map from the block index to (job, tile) and the
job's row of the table in place of the launch's arguments, and that is what the cases go after:

  (a) one job of one tile with a K tail;
  (b) three jobs of different shapes, reductions and leading dimensions (operands that are column windows of wider
      arrays), 1 + 4 + 3 tiles so that no job starts on a multiple of 8 tiles, one job's state a view at a non-zero,
      256-byte-aligned offset of a larger bucket;
  (c) eight jobs of 72 tiles: 576 tiles, more than the chip's 512 workgroup slots, so a second round exists and job
      boundaries fall inside rounds;
  (d) one job of several tiles: the grouped entry point equals the ungrouped one.

Arguments the entry point refuses leave the state untouched, and the launch-free query that the scheduler asks
(sei_gemm_bf16nt_dw2_adam_groupable) answers without a GPU.
"""
import ctypes

import pytest
import torch

gpu = pytest.mark.gpu

WIDE, LOOP = 16, 1
LR, BETA1, BETA2, EPS = 2e-4, 0.9, 0.99, 1e-8
BAD_ARG = 10001


@pytest.fixture(scope="module")
def N():
    import _native
    return _native


class Job:
    """Operands and start state of one job. pad: extra columns of the arrays the operands are windows of (leading dimensions
    M + pad / N + pad, the window starting `pad` columns in); bucket_offset: the state lives that many elements into a
    larger flat array (a multiple of 64 floats = 256 bytes; the bf16 copy then starts on 128 bytes)."""

    def __init__(self, M, Nn, K1, K2, seed, pad=0, bucket_offset=0):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        self.M, self.N, self.K1, self.K2 = M, Nn, K1, K2
        self.lda, self.ldb = M + pad, Nn + pad
        self.A = [(0.05 * torch.randn((k, self.lda), device="cuda", generator=gen)).bfloat16() for k in (K1, K2)]
        self.B = [torch.randn((k, self.ldb), device="cuda", generator=gen).bfloat16() for k in (K1, K2)]
        self.col = pad
        self.offset = bucket_offset
        self.start = (0.02 * torch.randn((M, Nn), device="cuda", generator=gen),
                      1e-3 * torch.randn((M, Nn), device="cuda", generator=gen),
                      1e-5 * torch.rand((M, Nn), device="cuda", generator=gen) + 1e-7)

    def fresh(self):
        """[param, exp_avg, exp_avg_sq, bf16 copy] as views of new flat arrays, plus those arrays (the tail past the views
        must stay as it was)."""
        n, off = self.M * self.N, self.offset
        flats = [torch.full((off + n + 64,), 7.0, device="cuda") for _ in range(3)]
        flats.append(torch.full((off + n + 64,), 7.0, device="cuda", dtype=torch.bfloat16))
        views = [f[off:off + n].view(self.M, self.N) for f in flats]
        for v, s in zip(views, self.start):
            v.copy_(s)
        views[3].zero_()
        return views, flats

    def pointers(self):
        return [t.data_ptr() + 2 * self.col for t in (*self.A, *self.B)]       # A1, A2, B1, B2


def hyper_of(N, wd, step):
    host = (ctypes.c_float * 6)()
    N.call("sei_adam_scalars", LR, BETA1, BETA2, EPS, wd, step, ctypes.cast(host, ctypes.c_void_p))
    return torch.tensor(list(host), device="cuda")


def table(N, jobs, states):
    rows = []
    for job, st in zip(jobs, states):
        a1, a2, b1, b2 = job.pointers()
        rows.append(N.AdamGemmJob(a1, a2, b1, b2, *[t.data_ptr() for t in st], job.lda, job.ldb, job.M, job.N, job.K1, job.K2))
    return (N.AdamGemmJob * len(rows))(*rows)


def run(N, jobs, wd, tile):
    """Two steps of every job; tile None: all jobs in one grouped launch per step, else each alone on `tile`."""
    fresh = [job.fresh() for job in jobs]
    states = [views for views, _ in fresh]
    for step in (5, 6):
        hyper = hyper_of(N, wd, step)
        if tile is None:
            N.call("sei_gemm_bf16nt_dw2_adam_group", table(N, jobs, states), len(jobs), hyper.data_ptr())
        else:
            for job, st in zip(jobs, states):
                a1, a2, b1, b2 = job.pointers()
                N.call("sei_gemm_bf16nt_dw2_adam_ex", a1, a2, job.lda, b1, b2, job.ldb, *[t.data_ptr() for t in st],
                       hyper.data_ptr(), job.M, job.N, job.K1, job.K2, tile)
    torch.cuda.synchronize()
    return fresh


def assert_same(got, want, what):
    for j, ((gv, gf), (wv, wf)) in enumerate(zip(got, want)):
        for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), gf, wf):      # the whole flat arrays: views and what surrounds them
            assert torch.equal(a, b), (what, j, name, int((a != b).sum()))
        assert torch.equal(gf[3].view(torch.int16), wf[3].view(torch.int16)), (what, j, "bf16 copy")


CASES = {
    "a_one_tile_k_tail": lambda: [Job(128, 256, 64, 32, seed=1)],
    "b_mixed_shapes": lambda: [Job(128, 256, 40, 24, seed=2, pad=8),
                               Job(256, 512, 192, 96, seed=3, pad=64, bucket_offset=192),
                               Job(384, 256, 8, 8, seed=4)],
    "c_second_round": lambda: [Job(1152, 2048, 64, 32, seed=10 + j) for j in range(8)],
    "d_one_job": lambda: [Job(384, 768, 104, 96, seed=5, pad=16)],
}


@gpu
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("case", sorted(CASES))
def test_grouped_launch_equals_every_job_alone(N, case, wd):
    jobs = CASES[case]()
    for job in jobs:
        assert N.adam_gemm_plan(job.M, job.N, job.K1, job.K2, WIDE) == ("nt", 128, 256, 1)
        assert N.adam_gemm_plan(job.M, job.N, job.K1, job.K2, LOOP) == ("nt", 128, 128, 1)
    grouped = run(N, jobs, wd, None)
    for (views, _), job in zip(grouped, jobs):
        assert float((views[0] - job.start[0]).abs().max()) > 1e-5               # the steps moved every job's parameter
    assert_same(grouped, run(N, jobs, wd, WIDE), "grouped vs each job alone on the 128 x 256 tile")
    assert_same(grouped, run(N, jobs, wd, LOOP), "grouped vs each job alone on the 128 x 128 loop")


@gpu
def test_refused_arguments_launch_nothing(N):
    """0 and 9 jobs, N % 256 != 0, a parameter off its 16-byte boundary, two jobs on the same state: SEI_ERR_BAD_ARG, and
    no element of any state array changes."""
    jobs = [Job(128, 256, 64, 32, seed=21), Job(256, 256, 64, 32, seed=22)]
    fresh = [job.fresh() for job in jobs]
    states = [views for views, _ in fresh]
    before = [[f.clone() for f in flats] for _, flats in fresh]
    hyper = hyper_of(N, 0.01, 5)
    group = N.lib().sei_gemm_bf16nt_dw2_adam_group

    def refused(arr, n):
        return group(arr, n, hyper.data_ptr(), N.stream()) == BAD_ARG

    good = table(N, jobs, states)
    assert refused(good, 0)
    nine = (N.AdamGemmJob * 9)(*([good[0]] * 9))
    assert refused(nine, 9)
    narrow = table(N, jobs, states)
    narrow[1].N, narrow[1].ldb = 128, 128                                        # whole 128 x 128 tiles, no 128 x 256 ones
    assert refused(narrow, 2)
    ragged = table(N, jobs, states)
    ragged[0].M, ragged[0].lda = 64, 64
    assert refused(ragged, 2)
    shifted = table(N, jobs, states)
    shifted[1].param = states[1][0].data_ptr() + 4
    assert refused(shifted, 2)
    odd_k = table(N, jobs, states)
    odd_k[0].K2 = 28
    assert refused(odd_k, 2)
    overlap = table(N, jobs, states)
    overlap[1].exp_avg = states[0][1].data_ptr() + 16 * 256                      # inside job 0's exp_avg
    assert refused(overlap, 2)
    torch.cuda.synchronize()
    for (_, flats), kept in zip(fresh, before):
        for a, b in zip(flats, kept):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert group(good, 2, hyper.data_ptr(), N.stream()) == 0                     # and the table they were derived from runs
    torch.cuda.synchronize()
    assert not torch.equal(fresh[1][0][0], jobs[1].start[0])


def test_groupable_query_runs_without_a_gpu():
    """Host arithmetic: the step's six level-3 weight gradients are groupable (whole 128 x 256 tiles, one round of
    workgroups each), the bottleneck pair (16 rounds) is not, and neither is a shape the wide tile does not fit."""
    import _native
    for M, Nn, K1, K2 in ((2048, 8192, 2304, 1152), (8192, 2048, 2304, 1152), (8192, 2048, 576, 288)):
        assert _native.adam_gemm_groupable(M, Nn, K1, K2)
    for M, Nn in ((8192, 32768), (32768, 8192)):
        assert not _native.adam_gemm_groupable(M, Nn, 576, 288)
    assert not _native.adam_gemm_groupable(2048, 8192 + 128, 2304, 1152)         # N % 256 != 0
    assert not _native.adam_gemm_groupable(2048 + 64, 8192, 2304, 1152)          # M % 128 != 0
    assert not _native.adam_gemm_groupable(2048, 8192, 2304, 1150)               # a reduction the GEMM refuses
    assert _native.adam_gemm_groupable(128, 256, 64, 32)
