"""CPU tests of the host layer: flags, crop quirk, samplers, schedules, checkpoints, band builders,
resampler matrices, and the N>1 gradient exchange over gloo (world_size 2)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from oracle import closed_form as cf
from oracle import torch_path as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_kernel_table_matches_golden(golden):
    """float64 to the last few bits: the CPU's vector width changes `exp` and the order of the normalising sum (by up to
    8 ulp for a sequential 169-term sum), so the golden is bit for bit only on the host that generated it."""
    import physics
    g = golden("g1_kernels")
    for name in g.files:
        k = physics.get_kernel(name)
        assert k.dtype == torch.float64
        np.testing.assert_allclose(k.numpy(), g[name], rtol=1e-14, atol=0)
        t = physics.kernels.taps_1d(name)
        np.testing.assert_allclose(torch.outer(t, t).numpy() / float(t.sum()) ** 2, g[name], rtol=1e-14, atol=0)
    with pytest.raises(AssertionError):
        physics.get_kernel("Box_R9")
    bk = physics.BlurKernel("Gaussian_R2").to_tensor("cpu")
    assert tuple(bk.shape) == (1, 1, 13, 13) and bk.dtype == torch.float64


def test_blur_kernel_from_file(tmp_path):
    import physics
    k = torch.rand(5, 5, dtype=torch.float64)
    path = str(tmp_path / "k.pt")
    torch.save(k, path)
    assert torch.equal(physics.BlurKernel(path).to_tensor("cpu")[0, 0], k)


def test_band_matrices_match_closed_form():
    from physics import _bands
    for n, r in [(96, 2), (96, 3), (96, 4), (48, 4), (130, 2)]:
        dense = _bands.aa_bicubic_matrix(n, 1 / r)
        np.testing.assert_allclose(dense, cf.aa_weights(n, r), atol=1e-15)
        for mat in (dense, dense.T):
            w, lo, nb, step = _bands.to_band(np.ascontiguousarray(mat))
            rebuilt = np.zeros_like(mat)
            for o in range(mat.shape[0]):
                n_ok = min(nb, mat.shape[1] - lo[o])
                rebuilt[o, lo[o]:lo[o] + n_ok] = w[o, :n_ok]
            np.testing.assert_allclose(rebuilt, mat, atol=1e-7)
            assert np.all(np.diff(lo) >= 0) and (np.diff(lo).max() if len(lo) > 1 else 0) == step
    for n, r in [(12, 2), (12, 3), (16, 4)]:
        np.testing.assert_allclose(_bands.plain_bicubic_matrix(n, r), cf.plain_bicubic_up_weights(n, r), atol=1e-15)
    # antialias pre-filter of the EI transform at rate 0.75 == torch's own antialiased resize
    x = torch.rand(1, 1, 48, 48, dtype=torch.float64)
    m = torch.from_numpy(_bands.aa_bicubic_matrix(48, 0.75))
    ref = torch.nn.functional.interpolate(x, scale_factor=0.75, mode="bicubic", antialias=True)
    assert (m @ x[0, 0] @ m.T - ref[0, 0]).abs().max() < 1e-12


def test_resampler_matrices_match_fft_oracle():
    from models import _mats
    for kind, H, W, r in [("down", 48, 48, 2), ("down", 16, 32, 2), ("up", 24, 24, 2), ("up", 12, 12, 4), ("up", 3, 3, 2)]:
        L1, R1, L2, R2 = (m.astype(np.float64) for m in _mats._host_matrices(kind, H, W, r))
        x = torch.rand(2, 3, H, W, dtype=torch.float64)
        ref = tp.ideal_downsample(x, r) if kind == "down" else tp.ideal_upsample(x, r)
        got = cf.sepmap2(x.numpy(), L1, R1, L2, R2)
        assert np.abs(got - ref.numpy()).max() < 5e-7
    with pytest.raises(RuntimeError):
        _mats._host_matrices("up", 16, 16, 3)


def test_crop_pair_reproduces_batched_quirk():
    import crop
    torch.manual_seed(3)
    x, y = torch.rand(2, 3, 256, 256), torch.rand(2, 3, 256, 256)
    torch.manual_seed(9)
    xc, yc = crop.CropPair("random", 48)(x, y, xy_size_ratio=1)
    torch.manual_seed(9)
    xr, yr = tp.crop_pair(x, y, 48, 1)
    assert torch.equal(xc, xr) and torch.equal(yc, yr)
    # offsets are drawn over the padded height 301 (quirk) unless the fix is requested
    pad = crop.MinSizePadding(48)(y)
    assert pad.shape == (2, 3, 301, 256)
    assert crop.MinSizePadding(48, fix_batched_crop=True)(y).shape == (2, 3, 256, 256)
    assert crop.MinSizePadding(48)(torch.rand(3, 30, 60)).shape == (3, 48, 60)      # 3-D item: as intended
    xs, ys = crop.CropPair("center", 48)(torch.rand(3, 200, 200), torch.rand(3, 100, 100))
    assert xs.shape == (3, 96, 96) and ys.shape == (3, 48, 48)


def test_scale_parameter_draws_match_reference(golden):
    import transforms
    g = golden("g4_scale_transform")
    for k in range(4):
        torch.manual_seed(k)
        r, c = transforms.sample_downsampling_parameters(4, "cpu", torch.float32, [0.75, 0.5])
        np.testing.assert_array_equal(r.numpy(), g[f"draw.seed{k}.rate"])
        np.testing.assert_array_equal(c.numpy(), g[f"draw.seed{k}.center"])


def test_lr_schedules_match_reference():
    import warnings
    import scheduler
    want = json.load(open(os.path.join(GOLDEN, "g9_lr_schedule.json")))
    for key, lrs in want.items():
        kind, epochs = key.rsplit(".", 1)
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.Adam([p], lr=1e-4)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sch = scheduler.get_lr_scheduler(opt, int(epochs), kind)
            got = []
            for _ in range(int(epochs)):
                got.append(opt.param_groups[0]["lr"])
                opt.step()
                sch.step()
        np.testing.assert_allclose(got, lrs, rtol=1e-12)
    with pytest.raises(ValueError):
        scheduler.get_lr_scheduler(opt, 10, "nope")


def test_flags_and_defaults_match_reference():
    sys.path.insert(0, ROOT)
    import train
    a = train.build_parser().parse_args(["--task", "deblurring", "--method", "proposed", "--out_dir", "o"])
    assert (a.device, a.noise_level, a.batch_size, a.Loss__crop_size) == ("cpu", 5, 8, 48)
    assert a.ProposedModel__architecture == "Transformer" and a.physics_v2 and a.ProposedLoss__stop_gradient
    assert a.ConvolutionalModel__hidden_channels == 32 and a.ConvolutionalModel__scales == 5
    assert a.sure_averaged_cst is None and a.sure_cropped_div and a.partial_sure and a.sure_margin is None
    assert a.ScalingTransform__kind == "padded" and not a.ScalingTransform__antialias
    assert a.lr_scheduler_kind == "delayed_linear_decay" and a.optimizer_beta2 == 0.999
    b = train.build_parser().parse_args(["--no-physics_v2", "--GroundTruthDataset__no_resize", "--download"])
    assert not b.physics_v2 and b.GroundTruthDataset__size is None and b.GroundTruthDataset__download


def test_state_dict_layout_and_seeded_init_match_reference():
    from models.convolutional import ConvolutionalModel
    man = json.load(open(os.path.join(GOLDEN, "g8_state_dict_manifest.json")))
    for tag, up in [("deblur", 1), ("sr2", 2), ("sr4", 4)]:
        with torch.device("meta"):
            m = ConvolutionalModel(in_channels=3, upsampling_rate=up, residual=True, inner_residual=True,
                                   num_conv_blocks=1, hidden_channels=32, inout_convs=True, scales=5)
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == man[tag]["keys"]
        assert sum(p.numel() for p in m.parameters()) == man[tag]["num_parameters"]
    g = np.load(os.path.join(GOLDEN, "g7_unet_h8s3_deblur.npz"))
    torch.manual_seed(0)
    m = ConvolutionalModel(in_channels=3, upsampling_rate=1, residual=True, inner_residual=True,
                           num_conv_blocks=1, hidden_channels=8, inout_convs=True, scales=3)
    for k, v in m.state_dict().items():
        if ".ln." not in k:                       # the golden's norm parameters were perturbed after init
            np.testing.assert_array_equal(v.numpy(), g["sd." + k])


def test_checkpoint_format(tmp_path):
    import training

    class M:
        def get_weights(self):
            return {"seq.0.in_conv.weight": torch.ones(2)}

    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=1e-4)
    sch = torch.optim.lr_scheduler.LinearLR(opt)
    path = str(tmp_path / "a" / "ckp_1.pt")
    training.save_training_state(0, M(), opt, sch, path)
    st = torch.load(path)
    assert set(st) == {"epoch", "params", "optimizer", "scheduler"}
    assert torch.equal(training.get_weights(path, "cpu")["seq.0.in_conv.weight"], torch.ones(2))


def test_fused_adam_state_interchanges_with_torch_adam():
    """FlatAdam.state_dict() / load_state_dict() speak torch.optim.Adam's per-parameter layout over
    model.parameters() (what the reference checkpoints under "optimizer", src/training.py:23-31), so --RESUME
    works across the reference, --no-fused_optimizer and --fused_optimizer runs."""
    from models.convolutional import ConvolutionalModel
    from optim import FlatAdam
    torch.manual_seed(0)
    m = ConvolutionalModel(in_channels=3, upsampling_rate=2, residual=True, inner_residual=True, num_conv_blocks=1,
                           hidden_channels=8, inout_convs=True, scales=3)
    m.flatten_parameters()
    ref = torch.optim.Adam(m.parameters(), lr=3e-4, betas=(0.9, 0.99))
    sch = torch.optim.lr_scheduler.LinearLR(ref)                   # adds "initial_lr" to the group, as training does
    for p in m.parameters():
        p.grad = torch.randn_like(p)
    ref.step()
    ref.step()
    fused = FlatAdam(m, lr=1e-4)
    assert fused.state_dict()["state"] == {}                       # torch's Adam has no state before a step either
    fused.load_state_dict(ref.state_dict())
    st = fused.state[m.flat_params]
    assert st["step"] == 2 and fused.param_groups[0]["lr"] == ref.param_groups[0]["lr"]
    assert fused.param_groups[0]["betas"] == (0.9, 0.99) and "initial_lr" in fused.param_groups[0]
    p0 = next(iter(m.parameters()))
    off = (p0.data_ptr() - m.flat_params.data_ptr()) // 4
    assert torch.equal(st["exp_avg"][off:off + p0.numel()].view(p0.shape), ref.state[p0]["exp_avg"])
    back = torch.optim.Adam(m.parameters(), lr=1.0)
    back.load_state_dict(fused.state_dict())                       # and the way back, into a plain torch Adam
    a, b = ref.state_dict(), back.state_dict()
    assert a["param_groups"][0].keys() == b["param_groups"][0].keys()
    assert all(torch.equal(a["state"][i][k], b["state"][i][k]) for i in a["state"] for k in a["state"][i])
    bad = ref.state_dict()
    bad["param_groups"][0]["params"] = bad["param_groups"][0]["params"][:-1]
    with pytest.raises(ValueError, match="parameters"):
        fused.load_state_dict(bad)


def test_device_cache_shards_have_equal_length():
    """Every rank of a multi-GPU run holds the same number of cached pairs (wrap-around padding, as torch's
    DistributedSampler): ranks that run different numbers of steps would hang in the all-reduce."""
    from datasets.device_cache import DeviceResidentPairs

    class Items:
        deterministic_measurements = True

        def __len__(self):
            return 7

        def __getitem__(self, i):
            return torch.full((3, 8, 8), float(i)), torch.full((3, 8, 8), float(i))

    class P:
        task = "deblurring"

    shards = [DeviceResidentPairs(Items(), P(), crop_size=8, rank=r, world=3) for r in range(3)]
    assert [len(s) for s in shards] == [3, 3, 3]
    seen = sorted(int(x[0, 0, 0]) for s in shards for x, _ in s.pairs)
    assert seen == [0, 0, 1, 1, 2, 3, 4, 5, 6]
    assert len(list(shards[0].batches(2))) == len(list(shards[2].batches(2))) == 2


def test_psnr_metric():
    import metrics
    a, b = torch.rand(3, 20, 20), torch.rand(3, 20, 20)
    assert abs(float(metrics.psnr_fn(a, b)) - float(tp.psnr_y(a, b))) < 1e-5
    assert float(metrics.psnr_fn(a, a + 1e-3)) == pytest.approx(60.0, abs=1e-3)


# ------------------------------------------------------------------ N>1 over gloo
def _reducer_worker(rank, world, port, numel, chunk_mib, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))
    import torch.distributed as dist
    import parallel
    r, _, w = parallel.init_from_env(backend="gloo")
    g = torch.Generator().manual_seed(100 + r)
    grads = torch.randn(numel, generator=g)
    params = torch.full((numel,), float(r))
    parallel.broadcast_parameters(params)
    red = parallel.FlatGradientReducer(grads, chunk_mib=chunk_mib)
    red.reduce_async()
    for k in range(len(red.bounds)):
        red.wait(k)
    # bf16-compressed exchange: the f32 bucket is left alone, the reduced values land in red16.comm
    g2 = torch.randn(numel, generator=torch.Generator().manual_seed(200 + r))
    red16 = parallel.FlatGradientReducer(g2, chunk_mib=chunk_mib, comm_dtype=torch.bfloat16)
    red16.reduce_async()
    red16.wait_all()
    want16 = sum(torch.randn(numel, generator=torch.Generator().manual_seed(200 + k)).bfloat16().float() for k in range(w))
    assert red16.comm.dtype == torch.bfloat16 and (red16.comm.float() - want16).abs().max() < 0.05
    # slices the producer writes into the bf16 exchange buffer itself (direct ranges): the cast skips them after a step
    # that did so, and casts them as usual after one that did not (an eager step)
    g4 = torch.randn(numel, generator=torch.Generator().manual_seed(400 + r))
    red_d = parallel.FlatGradientReducer(g4, chunk_mib=chunk_mib, comm_dtype=torch.bfloat16)
    red_d._chunk = 200_000
    red_d.set_early_range((300_000, 700_004))
    direct = [(300_000, 500_000), (600_000, 700_000)]
    red_d.set_direct_ranges(direct)
    for lo, hi in direct:                                 # what the weight-gradient GEMMs would have stored
        red_d.comm[lo:hi] = float(r + 1)
    g4_marked = g4.clone()
    for lo, hi in direct:
        g4[lo:hi] = 1000.0                                # the float32 bucket holds junk there: it must not be cast
    red_d.reduce_async(direct=True)
    red_d.wait_all()
    got = red_d.comm.float()
    want4 = sum(torch.randn(numel, generator=torch.Generator().manual_seed(400 + k)).bfloat16().float() for k in range(w))
    for lo, hi in direct:
        assert float((got[lo:hi] - sum(range(1, w + 1))).abs().max()) == 0.0
        want4[lo:hi] = got[lo:hi]
    assert (got - want4).abs().max() < 0.05
    g4.copy_(g4_marked)
    red_d.reduce_async(direct=False)                      # an eager step: everything comes from the float32 bucket
    red_d.wait_all()
    want4e = sum(torch.randn(numel, generator=torch.Generator().manual_seed(400 + k)).bfloat16().float() for k in range(w))
    assert (red_d.comm.float() - want4e).abs().max() < 0.05
    # reduce-scatter + all-gather mode: same sums; the ragged last chunk falls back to all_reduce
    g3 = torch.randn(numel, generator=torch.Generator().manual_seed(300 + r))
    red_rs = parallel.FlatGradientReducer(g3, chunk_mib=chunk_mib, mode="rs_ag")
    red_rs.reduce_async()
    red_rs.wait_all()
    want3 = sum(torch.randn(numel, generator=torch.Generator().manual_seed(300 + k)) for k in range(w))
    assert (g3 - want3).abs().max() < 1e-6 and len(red_rs._shards) == len(red_rs.bounds) - 1
    loss = parallel.all_reduce_mean_scalar(torch.tensor(float(r + 1)))
    want = sum(torch.randn(numel, generator=torch.Generator().manual_seed(100 + k)) for k in range(w))
    # plain floats only: tensors sent through the queue would outlive this process's shared memory
    q.put((r, float((grads - want).abs().max()), float(params.abs().max()), float(loss), len(red.bounds)))
    dist.destroy_process_group()


def test_flat_gradient_reducer_gloo_world2():
    import torch.multiprocessing as mp
    sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))
    import parallel
    assert parallel.chunk_bounds(10, 4) == [(0, 4), (4, 8), (8, 10)]
    numel = 1_000_003
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + os.getpid() % 2000
    procs = [ctx.Process(target=_reducer_worker, args=(r, 2, port, numel, 1, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r, grad_err, param_max, loss, nchunks in res:
        assert grad_err < 1e-6                     # every rank holds the sum of both ranks' gradients
        assert param_max == 0                      # rank 0's weights everywhere
        assert loss == pytest.approx(1.5) and nchunks == 4


def _sharded_worker(r, w, port, q):
    """One rank of the sharded optimizer step on CPU tensors over gloo: parallel.FlatGradientReducer in mode "sharded"
    (what optim.FlatAdam turns "rs_ag" into) + FlatAdam._step_sharded / consolidate with a torch restatement of the
    Adam kernel as the update function (the product's update is the HIP kernel: no CPU path)."""
    import torch
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, "scale-equivariant-imaging_amd"))
    import parallel
    from models import _ops
    from models._flat import FlatParameterBucket
    from optim import FlatAdam
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE=str(w), LOCAL_RANK=str(r))
    parallel.init_from_env(backend="gloo")

    class Net(FlatParameterBucket, torch.nn.Module):
        def __init__(self):
            super().__init__()
            g = torch.Generator().manual_seed(5)
            mk = lambda *s: torch.nn.Parameter(torch.randn(s, generator=g))
            self.big = mk(96, 64, 1, 1)            # read through its bf16 copy only (both extents % 32 == 0)
            self.small = mk(40, 3, 1, 1)           # a 1x1 weight some float32 path reads
            self.bias = mk(70)
            self.dw = mk(32, 1, 7, 7)
            self._init_bucket()
            self.flatten_parameters()

        def get_backbone(self):
            return self

    prev = _ops.set_compute_dtype("bf16")
    net = Net()
    total = net.flat_params.numel()
    assert net.flat_shadow_only_start == total - 96 * 64 and net.big.data_ptr() == net.flat_params[total - 6144:].data_ptr()
    net.flat_shadow = net.flat_params.bfloat16()
    start = net.flat_params.clone()
    red = parallel.FlatGradientReducer(net.flat_grads, chunk_mib=1, mode="rs_ag", comm_dtype=torch.float32)
    red._chunk = 2048                                   # several chunks on either side of the split
    opt = FlatAdam(net, lr=1e-2, reducer=red)
    assert red.mode == "sharded" and all(not (s < net.flat_shadow_only_start < e) for s, e in red.bounds)
    st = opt.state[net.flat_params]
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    grads = [[torch.randn(total, generator=torch.Generator().manual_seed(10 * step + k)) for k in range(w)]
             for step in range(2)]

    def adam(p, g, m, v, step):
        m.lerp_(g, 1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        p.addcdiv_(m, (v.sqrt() / (1 - b2 ** step) ** 0.5).add_(eps), value=-lr / (1 - b1 ** step))

    ref_p, ref_m, ref_v = start.clone(), torch.zeros(total), torch.zeros(total)
    stale_seen = False
    for step in (1, 2):
        net.flat_grads.copy_(grads[step - 1][r])
        red.reduce_async()
        st["step"] = step

        def update(lo, hi, g, g16):
            adam(net.flat_params[lo:hi], g.float() / w, st["exp_avg"][lo:hi], st["exp_avg_sq"][lo:hi], step)
            net.flat_shadow[lo:hi] = net.flat_params[lo:hi].bfloat16()

        opt._step_sharded(update, net.flat_shadow)
        adam(ref_p, sum(grads[step - 1]) / w, ref_m, ref_v, step)
        # the bf16 copies are complete on every rank, the head is complete in float32 ...
        first = net.flat_shadow_only_start
        assert torch.equal(net.flat_shadow[first:], ref_p[first:].bfloat16())
        assert torch.equal(net.flat_params[:first], ref_p[:first])
        # ... and the float32 masters of the OTHER rank's shares of the bf16-copy-only weights are not (by design)
        stale_seen = stale_seen or not torch.equal(net.flat_params[first:], ref_p[first:])
    assert stale_seen and opt._master_stale
    opt.consolidate()
    ok = (torch.equal(net.flat_params, ref_p) and torch.equal(st["exp_avg"], ref_m) and torch.equal(st["exp_avg_sq"], ref_v)
          and not opt._master_stale)
    sd = opt.state_dict()                                # torch.optim.Adam's layout, complete after consolidate()
    ok = ok and torch.equal(sd["state"][0]["exp_avg"].flatten(), ref_m[total - 6144:]) and len(sd["state"]) == 4
    full = None
    net.flat_grads.copy_(grads[0][r])
    red.reduce_async()
    full = red.gathered_gradient()
    ok = ok and torch.equal(full, grads[0][0] + grads[0][1])
    _ops.set_compute_dtype(prev)
    q.put((r, bool(ok), len(red.bounds), sum(red.is_sharded(k) for k in range(len(red.bounds)))))
    dist.destroy_process_group()


def test_sharded_optimizer_step_gloo_world2():
    """Two ranks, CPU + gloo: reduce-scatter of the gradient chunks, the step on each rank's shares, all-gather of the
    updated weights (bf16 copies alone for the GEMM weights) == one process stepping the whole bucket on the averaged
    gradient, bit for bit; `consolidate()` completes the float32 masters and the moments for a checkpoint."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r, ok, nchunks, nsharded in res:
        assert ok and nchunks >= 4 and nsharded >= nchunks - 1, (r, ok, nchunks, nsharded)


def test_reducer_chunk_plan_with_an_early_range():
    """Chunks never straddle the early range, cover the bucket exactly once, and the early ones come first in
    the consumption order."""
    import torch
    import parallel
    flat = torch.zeros(10_000)
    red = parallel.FlatGradientReducer(flat, chunk_mib=1)
    red._chunk = 1024                                   # small chunks for the test
    red.set_early_range((3000, 8200))
    assert red.bounds[0][0] == 0 and red.bounds[-1][1] == 10_000
    assert all(a[1] == b[0] for a, b in zip(red.bounds, red.bounds[1:]))
    assert all(not (s < 3000 < e or s < 8200 < e) for s, e in red.bounds)
    early = [k for k in range(len(red.bounds)) if 3000 <= red.bounds[k][0] < 8200]
    assert red.order[:len(early)] == early and sorted(red.order) == list(range(len(red.bounds)))
    red.set_early_range(None)
    assert red.order == list(range(len(red.bounds))) and red.bounds[0] == (0, 1024)
    # single process: reduce_async is a cast / no-op and wait() never blocks
    red.reduce_async()
    red.wait(0)
    red.wait_all()


# ------------------------------------------------------------------ N1: file-based data path (host side)
def _write_png(path, array):
    from PIL import Image
    Image.fromarray(array).save(path)


def test_png_decode_matches_the_file(tmp_path):
    """datasets._io.read_image restates torchvision.io.read_image (mode UNCHANGED): (C, H, W) uint8 with the
    file's own channel count."""
    import numpy as np
    import torch
    from datasets._io import read_image
    rng = np.random.default_rng(0)
    for name, shape in (("rgb", (37, 53, 3)), ("rgba", (20, 31, 4)), ("gray", (16, 9))):
        a = rng.integers(0, 256, size=shape, dtype=np.uint8)
        _write_png(tmp_path / f"{name}.png", a)
        t = read_image(str(tmp_path / f"{name}.png"))
        assert t.dtype == torch.uint8
        expect = a[:, :, None] if a.ndim == 2 else a
        assert t.shape == (expect.shape[2], expect.shape[0], expect.shape[1])
        assert np.array_equal(t.numpy().transpose(1, 2, 0), expect)


def test_resize_rule_and_filter_match_torch_antialiased_bicubic():
    """GroundTruthDataset's TF.resize(size=256, BICUBIC, antialias=True): torchvision's shorter-edge rule, then
    F.interpolate(size=...): the size-based band matrices reproduce torch's CPU result (float64) to 1e-12."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    from datasets.ground_truth import resized_hw
    from physics import _bands
    assert resized_hw(1356, 2040, 256) == (256, 385) and resized_hw(2040, 1356, 256) == (385, 256)
    assert resized_hw(256, 300, 256) == (256, 300) and resized_hw(100, 50, 256) == (512, 256)
    g = torch.Generator().manual_seed(3)
    for (h, w) in ((300, 421), (97, 64), (256, 513)):
        oh, ow = resized_hw(h, w, 256) if min(h, w) != 256 else (256, 300)
        x = torch.rand((1, 2, h, w), generator=g, dtype=torch.float64)
        ref = F.interpolate(x, size=(oh, ow), mode="bicubic", antialias=True, align_corners=False)
        Wv, Wh = _bands.aa_bicubic_matrix_to_size(h, oh), _bands.aa_bicubic_matrix_to_size(w, ow)
        mine = Wv @ x.numpy() @ Wh.T                       # (oh,h) @ (1,2,h,w) @ (w,ow)
        assert np.abs(mine - ref.numpy()).max() < 1e-12


def test_dataset_wrappers_follow_the_reference(tmp_path):
    """TestDataset crops x to a multiple of y; TrainingDataset crops pairs (css swaps in a re-degraded pair);
    get_dataset refuses what this build does not carry."""
    import types
    import pytest
    import torch
    import datasets

    class FakeSynthetic(torch.utils.data.Dataset):
        def __len__(self):
            return 2

        def __getitem__(self, i):
            return torch.arange(3 * 101 * 67, dtype=torch.float32).view(3, 101, 67), torch.ones(3, 50, 33)

    sr = types.SimpleNamespace(task="sr", rate=2)
    x, y = datasets.TestDataset(FakeSynthetic(), False, sr)[0]
    assert x.shape == (3, 100, 66) and y.shape == (3, 50, 33)
    torch.manual_seed(0)
    xt, yt = datasets.TrainingDataset(FakeSynthetic(), sr, False, False, None, True)[0]      # _HOTFIX crops
    assert xt.shape[-2:] == (96, 96) and yt.shape[-2:] == (48, 48)
    prep = datasets.PrepareTrainingPairs(types.SimpleNamespace(task="deblurring"), 32, "center")
    xc, yc = prep(torch.zeros(3, 64, 80), torch.zeros(3, 64, 80))
    assert xc.shape == (3, 32, 32) and yc.shape == (3, 32, 32)
    assert datasets.TestDataset(FakeSynthetic(), True, sr)[0][1].shape == (3, 50, 33)       # even-size trim: deblurring only
    args = types.SimpleNamespace(dataset="urban100", method="proposed", GroundTruthDataset__datasets_dir=str(tmp_path),
                                 GroundTruthDataset__download=False, GroundTruthDataset__size=256,
                                 GroundTruthDataset__split="train", memoize_gt=False,
                                 PrepareTrainingPairs__crop_size=256, PrepareTrainingPairs__crop_location="random",
                                 SingleImageDataset__image_path=None, SingleImageDataset__duplicates_count=4,
                                 SyntheticDataset__unique_seeds=True, SyntheticDataset__deterministic_measurements=True)
    phys = types.SimpleNamespace(task="deblurring")
    setattr(phys, "__manager", types.SimpleNamespace(task="deblurring"))
    with pytest.raises(NotImplementedError):
        datasets.get_dataset(args, "train", phys, "cpu")
    args.dataset = "div2k"
    with pytest.raises(FileNotFoundError):
        datasets.get_dataset(args, "train", phys, "cpu")
    with pytest.raises(ValueError):
        datasets.get_dataset(args, "validate", phys, "cpu")


def test_homogeneous_swinir_dataset_switches(monkeypatch):
    """HOMOGENEOUS_SWINIR (src/datasets/__init__.py:21-27,35-40,79-82; synthetic_dataset.py:43-53): 48-pixel same-size
    training crops, and the plain bicubic size-based interpolation matrix of the measurement upsampling against
    F.interpolate(size=..., mode="bicubic", align_corners=False) itself (float64, also for a non-integer ratio)."""
    import types
    import numpy as np
    import torch
    import torch.nn.functional as F
    import datasets
    from physics import _bands
    g = torch.Generator().manual_seed(4)
    for (h, w, oh, ow) in ((24, 30, 48, 60), (128, 192, 256, 385), (17, 16, 51, 49)):
        y = torch.rand((1, 2, h, w), generator=g, dtype=torch.float64)
        ref = F.interpolate(y, (oh, ow), mode="bicubic", align_corners=False)
        Wv, Wh = _bands.plain_bicubic_matrix_to_size(h, oh), _bands.plain_bicubic_matrix_to_size(w, ow)
        assert np.abs(Wv @ y.numpy() @ Wh.T - ref.numpy()).max() < 1e-12
    assert np.array_equal(_bands.plain_bicubic_matrix_to_size(24, 48), _bands.plain_bicubic_matrix(24, 2))

    class SameSize(torch.utils.data.Dataset):
        def __len__(self):
            return 1

        def __getitem__(self, i):
            return torch.rand(3, 100, 120), torch.rand(3, 100, 120)

    sr = types.SimpleNamespace(task="sr", rate=2)
    monkeypatch.setenv("HOMOGENEOUS_SWINIR", "1")
    prep = datasets.PrepareTrainingPairs(sr, 256, "random")
    assert prep.crop_size == 48
    xt, yt = datasets.TrainingDataset(SameSize(), sr, False, False, prep, True)[0]
    assert xt.shape == yt.shape == (3, 48, 48)
    monkeypatch.delenv("HOMOGENEOUS_SWINIR")
    assert datasets.PrepareTrainingPairs(sr, 256, "random").crop_size == 256


# ------------------------------------------------------------------ SwinIR (host side; parity unpinned, see the oracle)
def test_swinir_module_tree_matches_the_published_layout():
    """Parameter / buffer names, shapes and counts of the official SwinIR for the reference's constructor arguments
    (src/models/__init__.py:51-74): 11,504,163 parameters (deblurring), 11,752,487 (x2), 11,900,199 (x4); the oracle's
    functional state_dict has the same parameter keys; the mask buffer equals the oracle's shift mask."""
    from models.swinir import SwinIR
    from oracle import swinir_path as sp
    for up, count in ((1, 11_504_163), (2, 11_752_487), (4, 11_900_199)):
        torch.manual_seed(0)
        m = SwinIR(upscale=up, upsampler="pixelshuffle" if up > 1 else None)
        assert sum(p.numel() for p in m.parameters()) == count
        names = {k for k, _ in m.named_parameters()}
        ref = sp.swinir_init_state_dict(up)
        assert names == set(ref) and all(tuple(ref[k].shape) == tuple(m.state_dict()[k].shape) for k in ref)
    sd = m.state_dict()
    assert "layers.0.residual_group.blocks.0.attn_mask" not in sd
    assert torch.equal(sd["layers.0.residual_group.blocks.1.attn_mask"], sp.shift_mask(48, 48))
    assert torch.equal(sd["layers.5.residual_group.blocks.5.attn.relative_position_index"], sp.relative_position_index())
    rates = [b.drop_path_rate for b in m.blocks()]
    assert rates[0] == 0.0 and abs(rates[-1] - 0.1) < 1e-7 and np.allclose(rates, sp.drop_path_rates(), atol=1e-7)
    # Linear weights are re-initialised by trunc_normal(std 0.02), LayerNorm to (1, 0), as upstream's _init_weights
    w = sd["layers.2.residual_group.blocks.3.mlp.fc1.weight"]
    assert 0.015 < float(w.std()) < 0.025 and float(w.abs().max()) <= 2.0
    assert float(sd["norm.weight"].min()) == 1.0 and float(sd["layers.0.residual_group.blocks.0.attn.qkv.bias"].abs().max()) == 0.0
    m.eval()
    assert m.draw_drop_masks(4, "cpu") is None
    m.train()
    masks = m.draw_drop_masks(4, "cpu")
    assert masks[0] is None and len(masks) == 36
    assert all(abs(v) < 1e-6 or abs(v - 1 / 0.9) < 1e-5 for v in masks[-1][0].tolist())


def test_published_weight_files_load_into_the_default_backbone(tmp_path):
    """N2 (src/training.py:34-46, src/models/__init__.py:161-170): the authors' weight files are `backbone.state_dict()`
    of the deepinv SwinIR -- official parameter names plus the `attn_mask` / `relative_position_index` buffers -- stored
    bare or under "params".  A file with that key set (values from the oracle's seeded init; the network is not
    reachable from here) loads strictly through get_weights -> Model.load_weights, lands in the flat bucket, and
    get_weights() hands back the same keys, so files written here are readable upstream."""
    sys.path.insert(0, ROOT)
    import train
    import training
    from models import get_model
    from oracle import swinir_path as sp
    torch.manual_seed(1)
    published = dict(sp.swinir_init_state_dict(2))
    for i in range(6):
        for j in range(6):
            blk = f"layers.{i}.residual_group.blocks.{j}."
            published[blk + "attn.relative_position_index"] = sp.relative_position_index()
            if j % 2:
                published[blk + "attn_mask"] = sp.shift_mask(48, 48)
    a = train.build_parser().parse_args(["--task", "sr", "--sr_factor", "2", "--method", "proposed", "--out_dir", "o"])
    assert a.ProposedModel__architecture == "Transformer"
    for wrap in (False, True):
        path = str(tmp_path / f"Proposed_sr_x2_{int(wrap)}.pt")
        torch.save({"params": published} if wrap else published, path)
        model = get_model(a, physics=None, device="cpu")
        model.load_weights(training.get_weights(path, "cpu"))
        back = model.get_weights()
        assert set(back) == set(published)
        assert all(torch.equal(back[k], published[k]) for k in published)
        bb = model.get_backbone()
        w = model.get_parameter("model.model.conv_last.weight")            # the path demo/train.py:180-184 addresses
        assert w.data_ptr() == bb.conv_last.weight.data_ptr() and torch.equal(w, published["conv_last.weight"])
        bb.flatten_parameters()                                            # what .to(device) does
        w = model.get_parameter("model.model.conv_last.weight")
        lo = w.data_ptr() - bb.flat_params.data_ptr()
        assert 0 <= lo < bb.flat_params.numel() * 4 and torch.equal(w, published["conv_last.weight"])
    bad = dict(published)
    bad.pop("conv_last.bias")
    with pytest.raises(RuntimeError):
        model.load_weights(bad)


def test_noise2inverse_glue_matches_reference_golden(golden):
    """src/noise2inverse.py restated in noise2inverse.py against G12 (generated from the reference, tools/gen_golden.py):
    row slices through the FFT inverse filter, the X:1 (target, input) pair under numpy seed 3, and the summed
    reconstruction.  The Gaussian filter divides by ~1e-9: in float32 only the same FFT on the same host reproduces the
    values, so the fixture is float64, where any host's FFT agrees with it to ~1e-7."""
    import noise2inverse as n2i
    g = golden("g12_noise2inverse")
    y, k = torch.from_numpy(g["y"]), torch.from_numpy(g["kernel"])
    parts = n2i.ImageSlices(num_splits=4, task="deblurring", physics_filter=k, degradation_inverse_fn=None)(y)
    for j, part in enumerate(parts):
        np.testing.assert_allclose(part.numpy(), g[f"slice{j}"], rtol=1e-5, atol=0)
    masks = n2i.ImageSlices(4, "sr", None, lambda v: v).measurement_slices(y)
    assert torch.equal(sum(masks), y) and float(masks[1][:, :, 0::4].abs().max()) == 0.0
    assert torch.equal(masks[1][:, :, 1::4], y[:, :, 1::4])
    np.random.seed(3)
    tgt, inp = n2i.Noise2InverseTransform("deblurring", k, None)(None, y)
    assert int(g["pair.index"]) in range(4)
    np.testing.assert_allclose(tgt.numpy(), g["pair.tgt"], rtol=1e-5)
    np.testing.assert_allclose(inp.numpy(), g["pair.inp"], rtol=1e-5)
    model = n2i.Noise2InverseModel(lambda v: 0.25 * v + 0.1 * v * v, "deblurring", k, None)
    np.testing.assert_allclose(model(y).numpy(), g["model.x_hat"], rtol=1e-5)
    assert len(model.compute_inputs(y)) == 4
    up = n2i.ImageSlices(num_splits=4, task="sr", physics_filter=None, degradation_inverse_fn=lambda v: 2.0 * v)
    np.testing.assert_array_equal(up(y)[1].numpy(), g["sr.slice1"])
    # dataset wrappers: the training one ignores the flag, the test one trims deblurring measurements to even sizes
    import datasets

    class Pairs:
        def __getitem__(self, i):
            return torch.zeros(3, 9, 7), torch.ones(3, 9, 7)

        def __len__(self):
            return 1

    phys = type("P", (), {"task": "deblurring", "rate": 1})()
    x, yy = datasets.TestDataset(Pairs(), noise2inverse=True, physics=phys)[0]
    assert yy.shape == (3, 8, 6) and x.shape == (3, 8, 6)
    x, yy = datasets.TestDataset(Pairs(), noise2inverse=False, physics=phys)[0]
    assert yy.shape == (3, 9, 7)
    tr = datasets.TrainingDataset(Pairs(), phys, css=False, noise2inverse=True, prepare_training_pairs=lambda a, b: (a, b),
                                  _HOTFIX=False)
    assert tr[0][1].shape == (3, 9, 7) and tr.noise2inverse


def test_alignment_predicate_of_the_float4_kernels():
    """_native.aligned: the predicate the host layer routes on before sei_concat2_f32 / sei_scale_dev_f32 / sei_stack_axpy /
    sei_axpy / sei_split_bf16x2 (16-byte aligned operands); None is skipped, one misaligned operand is enough to refuse."""
    import _native as N
    base = torch.zeros(64 + 16)
    assert base.data_ptr() % 16 == 0
    assert N.aligned(base, None, base[4:], base[8:]) and N.aligned()
    for k in (1, 2, 3, 5):
        assert not N.aligned(base[k:]) and not N.aligned(base, base[k:])
    assert N.aligned(base[2:], to=8) and not N.aligned(base[1:], to=8)


@pytest.mark.parametrize("H,W", [(8, 8), (8, 24), (24, 8), (8, 16), (16, 8), (16, 16), (24, 16)])
def test_oracle_shift_mask_is_the_published_calculate_mask(H, W):
    """oracle/swinir_path.py::shift_mask against a literal transcription of SwinTransformerBlock.calculate_mask (the
    published slice loops, windows cut out one by one) for every shift 1..7 and for extents with a single window row or
    column, where slice(0, -8) is empty and there is no region 0 -- what a thin image gives after the forward's reflect
    padding. The coordinate form the attention kernels use (csrc/swin_kernels.hip: win_token) is held to the same
    tensor: a pair is masked, once, when its two region numbers differ."""
    from oracle import swinir_path as sp
    ws = 8
    for shift in range(1, ws):
        img_mask = torch.zeros((1, H, W, 1))
        h_slices = (slice(0, -ws), slice(-ws, -shift), slice(-shift, None))
        w_slices = (slice(0, -ws), slice(-ws, -shift), slice(-shift, None))
        cnt = 0
        for h in h_slices:
            for w in w_slices:
                img_mask[:, h, w, :] = cnt
                cnt += 1
        windows = [img_mask[0, y:y + ws, x:x + ws, 0].reshape(ws * ws) for y in range(0, H, ws) for x in range(0, W, ws)]
        mask_windows = torch.stack(windows)
        attn_mask = mask_windows.unsqueeze(1) - mask_windows.unsqueeze(2)
        attn_mask = attn_mask.masked_fill(attn_mask != 0, float(-100.0)).masked_fill(attn_mask == 0, float(0.0))
        got = sp.shift_mask(H, W, ws, shift)
        assert got.shape == (H // ws * (W // ws), ws * ws, ws * ws) and torch.equal(got, attn_mask), (H, W, shift)
        # the kernels' region arithmetic on shifted-frame coordinates (sy, sx)
        region = torch.empty((H // ws) * (W // ws), ws * ws)
        for win in range(region.shape[0]):
            wy, wx = divmod(win, W // ws)
            for i in range(ws * ws):
                sy, sx = wy * ws + (i >> 3), wx * ws + (i & 7)
                ry = 0 if sy < H - ws else (1 if sy < H - shift else 2)
                rx = 0 if sx < W - ws else (1 if sx < W - shift else 2)
                region[win, i] = 3 * ry + rx
        coord = torch.where(region.unsqueeze(1) != region.unsqueeze(2), -100.0, 0.0)
        assert torch.equal(coord, attn_mask), (H, W, shift)
        if H == ws:
            assert float(region.min()) >= 3                     # no region 0 .. 2: every window is a last-row window


def test_shadow_state_decides_when_a_bf16_copy_is_current():
    """models/_shadow.ShadowState on plain parameters: what a weight-generation bump, torch's version counters, the global
    bump and the stale range of a sharded optimizer step each do to "this bf16 copy may be used as it is"."""
    from models import _shadow
    from models._shadow import ShadowState
    a, b = ShadowState(), ShadowState()
    assert _shadow._new_plain_state is ShadowState and a.stale is None and a.transposed == {}
    p, q = torch.nn.Parameter(torch.zeros(4, 2, 1, 1)), torch.nn.Parameter(torch.zeros(3))
    for state in (a, b):
        for t in (p, q):
            state.note_version(t)
    assert not a.is_current() and not a.bucket_copy_current(p)          # nothing has written the bucket yet
    a.mark_current()
    b.mark_current()
    assert a.is_current() and a.bucket_copy_current(p) and a.bucket_copy_current(q)
    gen = a.generation()
    a.bump()                                                            # parameters changed, bf16 bucket not rewritten
    assert a.generation() != gen and not a.is_current() and not a.bucket_copy_current(p)
    assert b.is_current() and b.bucket_copy_current(p)                  # ... and model B is left alone
    a.bump(plain_shadow_written=True)                                   # the optimizer kernel rewrote the bucket as well
    assert a.is_current() and a.bucket_copy_current(p) and a.bucket_copy_current(q)
    with torch.no_grad():
        p.add_(1.0)                                                     # torch changed p behind the bucket's back
    assert not a.bucket_copy_current(p) and a.bucket_copy_current(q)
    assert not a.bucket_copy_current(torch.nn.Parameter(torch.zeros(2)))    # never looked at
    a.note_version(p)
    assert a.bucket_copy_current(p)

    class Model:
        pass
    model = Model()
    model._sei_plain_state = a
    _shadow.weights_updated(model, plain_shadow_written=True)
    assert a.is_current() and b.is_current() and _shadow.plain_shadow_is_current(model)
    _shadow.weights_updated(model)
    assert not a.is_current() and b.is_current()
    a.mark_current()
    _shadow.weights_updated()                                           # no model: every state is suspect
    assert not a.is_current() and not b.is_current() and not a.bucket_copy_current(q) and not b.bucket_copy_current(q)

    # the stale range of a sharded step: [offset, offset + numel) against [start, stop)
    p._sei_bucket_offset, numel = 64, p.numel()
    assert numel == 8 and not a.stale_overlaps(p)
    for span, hit in [((0, 64), False), ((0, 65), True), ((72, 100), False), ((71, 100), True), ((66, 67), True),
                      ((0, 1000), True), ((64, 72), True), ((0, 10), False), ((100, 200), False)]:
        _shadow.set_stale_masters(model, span)
        assert a.stale == span and a.stale_overlaps(p) is hit, span
    assert a.stale_overlaps(q)                                          # no known offset: it may lie inside
    assert "consolidate()" in str(a.stale_error())
    a.set_stale(None)
    assert a.stale is None and not a.stale_overlaps(p) and not a.stale_overlaps(q)


def test_lds_queries_of_the_resampler_and_the_separable_blur():
    """sei_resample_sepband_lds / sei_blur_sep_circ_lds: the dynamic LDS bytes of the launch the entry point would make
    (host arithmetic; the entry points size their launches with the same functions), 0 where it refuses. A DIV2K
    photograph resized as GroundTruthDataset does takes 105 KiB -- above the 64 KiB a kernel is launched with by default
    -- and a reduction by 8 halves its output tile instead of refusing."""
    import _native
    from physics import _bands
    L = _native.lib()

    def resample_lds(hi, wi, ho, wo):
        _, _, nbv, sv = _bands.to_band(_bands.aa_bicubic_matrix_to_size(hi, ho))
        _, _, nbh, sh = _bands.to_band(_bands.aa_bicubic_matrix_to_size(wi, wo))
        return (sv, nbv, sh, nbh), L.sei_resample_sepband_lds(hi, wi, ho, wo, nbv, sv, nbh, sh)

    assert resample_lds(1356, 2040, 256, 385) == ((6, 22, 6, 22), 107520)       # 112 x 208 footprint + 112 x 32 rows
    assert resample_lds(300, 421, 214, 300)[1] < 65536
    band, lds = resample_lds(260, 530, 33, 67)                                  # 152 x 280: 185 KiB with the 16 x 32 tile
    assert band == (8, 32, 8, 32) and lds == 4 * (152 * 152 + 152 * 16)         # ... the tile halved to 16 x 16
    assert L.sei_resample_sepband_lds(4000, 4000, 16, 32, 150, 250, 150, 250) == 4 * (150 * 150 + 150 * 1)   # down to 1 x 1
    assert L.sei_resample_sepband_lds(4000, 4000, 16, 32, 150, 250, 3000, 250) == 0     # one pixel's bands: 1.7 MiB
    assert L.sei_resample_sepband_lds(0, 8, 4, 4, 2, 1, 2, 1) == 0 and L.sei_resample_sepband_lds(8, 8, 4, 4, 0, 1, 2, 1) == 0
    assert L.sei_resample_sepband(16, 32, 1, 4000, 4000, 16, 32, 48, 64, 150, 250, 80, 96, 3000, 250, None) == 10002

    assert L.sei_blur_sep_circ_lds(63, 63, 64, 64) == 96272                     # 128 + 126 x 126 + 126 x 64 floats
    assert L.sei_blur_sep_circ_lds(19, 19, 256, 256) < 65536
    assert L.sei_blur_sep_circ_lds(36, 36, 64, 64) < 65536 < L.sei_blur_sep_circ_lds(37, 37, 64, 64)
    assert L.sei_blur_sep_circ_lds(63, 63, 5, 7) == 4 * (128 + ((67 * 69 + 3) & ~3) + 67 * 7)
    assert L.sei_blur_sep_circ_lds(64, 3, 64, 64) == 0 and L.sei_blur_sep_circ_lds(3, 64, 64, 64) == 0
    assert L.sei_blur_sep_circ_lds(0, 3, 64, 64) == 0 and L.sei_blur_sep_circ_lds(3, 3, 0, 64) == 0
    assert L.sei_blur_sep_circ(16, 32, 48, 64, 64, 3, 1, 64, 64, 0, None) == 10002
