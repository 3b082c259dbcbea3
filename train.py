#!/usr/bin/env python3
"""Training driver with the reference's command line (reference: demo/train.py).

    python train.py --device cuda --method proposed --task deblurring --kernel Gaussian_R2 \
        --ProposedModel__architecture Convolutional --dataset synthetic --out_dir runs/x --epochs 2

Same flags, defaults, epoch loop, csv log and checkpoint files as the reference; the arithmetic of the
step runs in libsei_hip.so. Differences, all build-side and documented in DESIGN.md:
  * multi-GPU = one process per GPU (`python -m torch.distributed.run --nproc-per-node N train.py ...`),
    gradients summed over RCCL; `--data_parallel_devices 0,1,..` (the reference's single-process
    nn.DataParallel) stops with the equivalent launch command. `--batch_size` is PER PROCESS: the reference's
    DataParallel splits one batch over the devices, here every rank draws its own batch, so the global batch
    is world x batch_size (pass batch_size / world to keep the reference's global batch and learning rate).
  * `--grad_comm_dtype bf16` halves the bytes of the gradient exchange (summed in bf16 across ranks; the
    default f32 keeps the exchange exact whatever the compute dtype).
  * `--fused_optimizer` (default on for Adam): one fused Adam kernel over the flat parameter bucket.
  * `--fix_batched_crop`: opt out of the reference's batched-crop padding quirk (crop.py).
  * the per-step `.item()` host sync of the reference is replaced by a device-side running mean.
  * `--task invert_a_tomography_like_filter` with the default `--partial_sure` needs `--sure_margin N` (or
    `--no-partial_sure`): the reference has no default margin for this task and stops on an unbound name.
  * `--fine_tuning` (demo/train.py:95-114, 144-186, 245-264): `--dataset DIR` trains on the measured PNGs of a folder
    (one random crop per file, kept on the device), the defaults become SGD at 1e-2, `--weights_distance_loss` keeps the
    weights near the loaded ones and `--fine_tuning_params` steps SwinIR's `conv_last` alone. With `--fused_optimizer`
    the SGD step and the penalty are one fused kernel (optim.FlatSGD) and the step replays from a hipGraph; so are,
    on one GPU, `--optimizer Adam`'s step and penalty (optim.FlatAdam with an anchor or frozen ranges; under several
    GPUs Adam with either fine-tuning option stays torch's own). With `--no-fused_optimizer` it is the reference's
    literal sequence (losses/weights_distance_loss.py + torch.optim.SGD / torch.optim.Adam).
    The reference's assertions are ValueErrors raised before anything touches the GPU; `--fine_tuning_params` with the
    Convolutional architecture, which has no `conv_last`, is one of them (the reference dies in `get_parameter`).
  * `--sure_unknown_noise` (UNSURE, restated from the paper; not in the reference): `--method proposed | sure` without a
    known noise level. The sigma^2 of the SURE term is a multiplier in device memory, started from
    `--unsure_init_noise_level` (default `--noise_level`) and moved by the loss kernel itself every step
    (`--unsure_step_size`, `--unsure_momentum`), so the step still replays from a hipGraph; the csv gets a third column
    `Estimated Noise Level` and the checkpoints a key `loss_state`, which `--RESUME` restores. One GPU.
    `--unsure_noise_model poisson_gaussian` estimates the two levels of Poisson-Gaussian noise (variance sigma^2 + gain *
    signal) instead: a second multiplier started from `--unsure_init_gain` and moved by `--unsure_gain_step_size`, a fourth
    csv column `Estimated Noise Gain`, eight floats in `loss_state`. `--noise_gain G` (settings.py) makes the synthetic
    measurements Poisson-Gaussian.
    `--unsure_init_from_measurements` (with a folder `--dataset DIR`): the multipliers start from the levels that
    noise_estimation.py reads off the loaded crops (the sei_noise_* kernels) instead of from a guess.
"""
import csv
import os
import random
import sys
from argparse import BooleanOptionalAction
from datetime import datetime
from os.path import isdir

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "scale-equivariant-imaging_amd"))

import crop  # noqa: E402
import graphs  # noqa: E402
import parallel  # noqa: E402
from datasets import get_dataset  # noqa: E402
from losses import check_unsure_args, get_loss  # noqa: E402
from models import get_model  # noqa: E402
from optim import FlatAdam, FlatSGD  # noqa: E402
from physics import get_physics  # noqa: E402
from scheduler import get_lr_scheduler  # noqa: E402
from settings import DefaultArgParser  # noqa: E402
from training import get_weights, save_training_state  # noqa: E402


def build_parser():
    parser = DefaultArgParser()
    flag, onoff = parser.add_argument, dict(action=BooleanOptionalAction)
    flag("--method", type=str)
    flag("--Loss__crop_training_pairs", default=True, **onoff)
    flag("--Loss__crop_size", type=int, default=48)
    flag("--ProposedLoss__transforms", type=str, default="Scaling_Transforms")
    flag("--ProposedLoss__stop_gradient", default=True, **onoff)
    flag("--ProposedLoss__sure_alternative", type=str, default=None)
    flag("--ProposedLoss__alpha_tradeoff", type=float, default=1.0)
    flag("--ScalingTransform__kind", type=str, default="padded")
    flag("--ScalingTransform__antialias", default=False, **onoff)
    flag("--out_dir", type=str)
    flag("--batch_size", type=int, default=8)
    flag("--epochs", type=int, default=None)
    flag("--checkpoint_interval", type=int, default=None)
    flag("--memoize_gt", default=True, **onoff)
    flag("--partial_sure", default=True, **onoff)
    flag("--sure_cropped_div", default=True, **onoff)
    flag("--sure_averaged_cst", default=None, **onoff)
    flag("--partial_sure_sr", default=False, **onoff)
    flag("--sure_margin", type=int, default=None)
    flag("--lr_scheduler_kind", type=str, default="delayed_linear_decay")
    flag("--optimizer_beta2", type=float, default=0.999)
    flag("--SyntheticDataset__deterministic_measurements", default=True, **onoff)
    flag("--GroundTruthDataset__split", type=str, default="train")
    flag("--weights", type=str, default=None)
    flag("--lr", type=float, default=None)
    flag("--optimizer", type=str, default=None)
    flag("--fine_tuning", default=False, **onoff)
    flag("--fine_tuning_params", default=False, **onoff)
    flag("--weights_distance_loss", default=False, **onoff)
    flag("--RESUME", type=str, default=None)
    # build-side additions
    flag("--fused_optimizer", default=True, **onoff)
    flag("--fix_batched_crop", default=False, **onoff)
    flag("--max_steps", type=int, default=None, help="stop each epoch after this many steps (smoke runs)")
    flag("--compute_dtype", choices=["f32", "bf16", "bf16x3"], default="f32",
         help="1x1-conv GEMM arithmetic: f32 (reference precision), bf16 MFMA with f32 accumulation, or bf16x3 (three bf16 "
              "MFMA products of head / remainder operands per float32 GEMM: 16 mantissa bits, held to the f32 parity bars)")
    flag("--hip_graph", default=True, **onoff)
    flag("--fuse_optimizer_step", default=True, **onoff,
         help="one GPU, bf16, hipGraph replay: weights of at least 2^24 elements (the U-Net's two deepest levels) take their "
              "Adam step in the epilogue of the GEMM that computes their gradient (optim.FlatAdam.fuse_weight_updates)")
    flag("--grad_comm_dtype", choices=["f32", "bf16"], default="f32",
         help="dtype of the all-reduced gradient bucket under torch.distributed.run: f32 (exact sum, default) or "
              "bf16 (half the xGMI bytes; the sum runs in bf16, its rounding grows with the number of ranks; "
              "needs --fused_optimizer)")
    flag("--grad_comm_mode", choices=["all_reduce", "rs_ag"], default="rs_ag",
         help="gradient exchange under torch.distributed.run: rs_ag = reduce-scatter of every chunk, the fused Adam steps "
              "this rank's 1 / world share and the UPDATED weights are all-gathered (sharded optimizer step; with another "
              "optimizer: reduce-scatter + all-gather of the gradients); all_reduce = chunked all-reduce, every rank "
              "steps the whole bucket (parallel.py, optim.py)")
    flag("--sure_unknown_noise", default=False, **onoff,
         help="UNSURE: --method proposed | sure without a known noise level. The sigma^2 in front of the SURE divergence "
              "becomes a multiplier in device memory that the loss kernel moves by gradient ascent every step; the csv "
              "gets a third column with the estimate (one GPU)")
    flag("--unsure_step_size", type=float, default=1e-4, help="ascent step of the multiplier (--sure_unknown_noise)")
    flag("--unsure_momentum", type=float, default=0.9, help="averaging of the ascent direction, in [0, 1)")
    flag("--unsure_init_noise_level", type=float, default=None,
         help="starting guess of the noise level on --noise_level's 0..255 scale (default: --noise_level, which keeps "
              "generating the synthetic measurements)")
    flag("--unsure_noise_model", choices=["gaussian", "poisson_gaussian"], default="gaussian",
         help="what --sure_unknown_noise estimates: one constant level, or (poisson_gaussian) the two levels of a variance "
              "sigma^2 + gain * signal, with a fourth csv column for the gain")
    flag("--unsure_init_gain", type=float, default=0.0,
         help="starting guess of the gain, in image units with images in [0, 1] (--unsure_noise_model poisson_gaussian)")
    flag("--unsure_gain_step_size", type=float, default=None,
         help="ascent step of the gain's multiplier (default: --unsure_step_size)")
    flag("--unsure_init_from_measurements", default=False, **onoff,
         help="start the multipliers of --sure_unknown_noise from the noise levels estimated on the measurements of the "
              "folder --dataset DIR (noise_estimation.py) instead of --unsure_init_noise_level / --unsure_init_gain")
    flag("--device_cache", default=False, **onoff,
         help="keep every (x, y) training pair in HBM (deterministic measurements) and draw crops on the device "
              "instead of the per-item DataLoader path (datasets/device_cache.py)")
    return parser


FINE_TUNING_PARAMS = ["model.model.conv_last.weight", "model.model.conv_last.bias"]       # demo/train.py:180-183


def check_fine_tuning_args(args):
    """The reference's assertions on the fine-tuning flags (demo/train.py:96-97, :179, :246), before any GPU object."""
    if args.dataset is not None and isdir(args.dataset):
        if not args.fine_tuning:
            raise ValueError("Datasets of predictors only are only supported for fine-tuning (--fine_tuning)")
        if args.method != "proposed":
            raise ValueError("Fine-tuning is only supported for the proposed method (--method proposed)")
    if args.fine_tuning_params and not args.fine_tuning:
        raise ValueError("Fine-tuning parameters are only supported for fine-tuning (--fine_tuning)")
    if args.weights_distance_loss and not args.fine_tuning:
        raise ValueError("Weights distance loss is only supported for fine-tuning (--fine_tuning)")
    if args.fine_tuning_params and args.ProposedModel__architecture != "Transformer":
        raise ValueError(f"--fine_tuning_params trains {FINE_TUNING_PARAMS[0]} and {FINE_TUNING_PARAMS[1]}: only "
                         "--ProposedModel__architecture Transformer has a conv_last, not "
                         f"{args.ProposedModel__architecture}")


UNSURE_FROM_FLAG = "--unsure_init_from_measurements"


def check_unsure_init_args(args):
    """What --unsure_init_from_measurements needs, refused by the flag's name before any GPU object exists."""
    if not args.unsure_init_from_measurements:
        return
    if not args.sure_unknown_noise:
        raise ValueError(f"{UNSURE_FROM_FLAG} starts the multipliers of --sure_unknown_noise: pass --sure_unknown_noise as well")
    if args.dataset is None or not isdir(args.dataset):
        raise ValueError(f"{UNSURE_FROM_FLAG} estimates the levels on measured data: --dataset must be a folder of PNG "
                         f"measurements, not {args.dataset!r} (synthetic measurements are made at --noise_level)")
    if args.unsure_init_noise_level is not None or args.unsure_init_gain != 0:
        raise ValueError(f"{UNSURE_FROM_FLAG} cannot be combined with an explicit --unsure_init_noise_level or "
                         "--unsure_init_gain: the start is either estimated or given")
    if args.RESUME is not None:
        raise ValueError(f"{UNSURE_FROM_FLAG} cannot be combined with --RESUME: a resumed run starts from the checkpoint's "
                         "loss_state")


def init_unsure_from_measurements(unsure, pairs, poisson_gaussian):
    """Estimate the noise levels over the loaded crops and write them into the UNSURE term's device state in place (a
    captured step reads the buffer's address): sigma^2, or eta and the gain."""
    from noise_estimation import NoiseEstimator
    estimator = NoiseEstimator(unsure.noise_state.device)
    for _, y in pairs:
        estimator.add(y)
    est = estimator.estimate()
    if not np.isfinite(est["sigma"]):
        raise ValueError(f"{UNSURE_FROM_FLAG}: no noise level could be read off the measurements (flags {est['flags']})")
    eta, gain = est["sigma"] ** 2, 0.0
    if poisson_gaussian:
        if est["model_ok"]:
            eta, gain = est["eta"], est["gain"]
        else:
            print(f"\n{UNSURE_FROM_FLAG}: the Poisson-Gaussian fit did not hold (flags {est['flags']}, "
                  f"{est['levels_used']} levels): starting from the Gaussian level and a gain of 0\n")
    with torch.no_grad():
        unsure.noise_state[0] = eta
        if poisson_gaussian:
            unsure.noise_state[4] = gain
    print(f"\nUNSURE starts from the measurements ({est['quads']} quads of {len(pairs)} crops): noise level "
          f"{255 * eta ** 0.5:.3f}" + (f", gain {gain:.5f}" if poisson_gaussian else "") + "\n")
    return est


def _crop_offsets(height, width, size):
    """torchvision's RandomCrop.get_params: two CPU-generator draws, none when the image is exactly the crop."""
    if height < size or width < size:
        raise ValueError(f"Required crop size {(size, size)} is larger than input image size {(height, width)}")
    if height == size and width == size:
        return 0, 0
    i = torch.randint(0, height - size + 1, size=(1,)).item()
    j = torch.randint(0, width - size + 1, size=(1,)).item()
    return i, j


def measurement_folder(path, crop_size, device):
    """demo/train.py:98-114: every *.png of a folder as a measurement y in [0, 1] (three channels), one random
    `crop_size` crop per file drawn at load time, kept on the device; x is a dummy of zeros that the loss never reads
    (cropped separately, as the reference does: the same draws from the CPU generator)."""
    from glob import glob
    from datasets._io import read_image
    pairs = []
    for f in glob(os.path.join(path, "*.png")):
        y = read_image(f).to(device).float() / 255.0
        y = y[:3, :, :]                                       # discard the alpha channel if it exists
        _crop_offsets(y.shape[1], y.shape[2], crop_size)      # x's own crop of zeros
        i, j = _crop_offsets(y.shape[1], y.shape[2], crop_size)
        y = y[:, i:i + crop_size, j:j + crop_size].contiguous()
        pairs.append((torch.zeros_like(y), y))
    return pairs


def main(argv=None):
    rank, local_rank, world = parallel.init_from_env()
    seed = 0 + rank                                   # reference: all seeds 0 (single process)
    torch.manual_seed(0)                              # identical initial weights on every rank
    np.random.seed(seed)
    random.seed(seed)

    args = build_parser().parse_args(argv)
    if args.device == "cuda" and world > 1:
        args.device = f"cuda:{local_rank % torch.cuda.device_count()}"     # (% only matters for shared-GPU rehearsals)
        torch.cuda.set_device(args.device)
    check_fine_tuning_args(args)
    check_unsure_args(args, world)
    check_unsure_init_args(args)
    crop.FIX_BATCHED_CROP = args.fix_batched_crop

    physics = get_physics(args, device=args.device)
    model = get_model(args=args, physics=physics, device=args.device)
    model.to(args.device)
    model.train()
    if args.weights is not None:
        model.load_weights(get_weights(args.weights, args.device))
    backbone = model.get_backbone()
    parallel.broadcast_parameters(backbone.flat_params)       # (no-op without a gradient exchange)
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)                      # decorrelated b / noise / rates / centres per rank

    loss = get_loss(args=args, physics=physics)
    unsure = loss.unsure_term()                       # the SURE term that owns the estimated noise level, or None
    unsure_pg = unsure is not None and args.unsure_noise_model == "poisson_gaussian"       # ... and the estimated gain
    if unsure is not None:
        unsure.to(args.device)
    if isdir(args.dataset):
        dataset = measurement_folder(args.dataset, args.PrepareTrainingPairs__crop_size, args.device)
        if args.unsure_init_from_measurements:
            init_unsure_from_measurements(unsure, dataset, unsure_pg)
    else:
        dataset = get_dataset(args=args, purpose="train", physics=physics, device=args.device,
                              _HOTFIX=(args.task == "sr"))
    sampler = None
    if world > 1:
        sampler = torch.utils.data.distributed.DistributedSampler(dataset, shuffle=True, seed=0)
    dataloader = torch.utils.data.DataLoader(dataset, batch_size=args.batch_size, shuffle=sampler is None,
                                             sampler=sampler)
    device_cache = None
    if args.device_cache:
        if args.method == "css" or not args.SyntheticDataset__deterministic_measurements:
            raise ValueError("--device_cache needs deterministic measurements (and no css re-degradation)")
        if isdir(args.dataset):
            raise ValueError("--device_cache holds (x, y) pairs of a dataset; a folder of measurements is on the device already")
        from datasets import SyntheticPairs
        from datasets.device_cache import DeviceResidentPairs
        if isinstance(dataset, SyntheticPairs):
            full = SyntheticPairs(physics, args.device, length=len(dataset))
        else:
            full = dataset.dataset.synthetic_dataset
        device_cache = DeviceResidentPairs(full, physics, crop_size=args.PrepareTrainingPairs__crop_size,
                                           crop_location=args.PrepareTrainingPairs__crop_location,
                                           hotfix_sr_crop=(args.task == "sr"), rank=rank, world=world)
        if rank == 0:
            print(f"\nDevice cache: {len(device_cache)} pairs, {device_cache.nbytes() / 2**20:.0f} MiB\n")

    epochs = args.epochs if args.epochs is not None else {"urban100": 4000, "ct": 100}.get(args.dataset, 500)
    if args.lr is not None:
        lr = args.lr
    elif args.fine_tuning:
        lr = 1e-2
    else:
        lr = 2e-4 if args.task == "sr" else 1e-4
    optimizer_kind = args.optimizer if args.optimizer is not None else ("SGD" if args.fine_tuning else "Adam")
    if rank == 0:
        print(f"\nSelected learning rate: {lr:e}\n")
        print(f"\nSelected optimizer: {optimizer_kind}\n")

    from models import _ops as model_ops
    model_ops.set_compute_dtype(args.compute_dtype)
    # FlatAdam's penalty and frozen ranges need the complete gradient on this GPU (sei_adam_anchor_fused); the exchange's
    # per-chunk and sharded steps know neither: under several GPUs Adam with either fine-tuning option is torch's own
    fine_tuning_option = bool(args.fine_tuning_params or args.weights_distance_loss)
    fused_adam = optimizer_kind == "Adam" and args.fused_optimizer and not fine_tuning_option
    fused_adam_fine_tuning = (optimizer_kind == "Adam" and args.fused_optimizer and fine_tuning_option
                              and not parallel.exchange_active())
    if args.grad_comm_dtype == "bf16" and not fused_adam:
        raise ValueError("--grad_comm_dtype bf16 needs the fused Adam (it reads the bf16 bucket directly)")
    comm_dtype = torch.bfloat16 if args.grad_comm_dtype == "bf16" else torch.float32
    reducer = parallel.FlatGradientReducer(backbone.flat_grads, comm_dtype=comm_dtype,
                                           mode=args.grad_comm_mode) if parallel.exchange_active() else None
    only = FINE_TUNING_PARAMS if args.fine_tuning_params else None
    params = model.parameters() if only is None else [model.get_parameter(key) for key in only]
    if fused_adam:
        optimizer = FlatAdam(model, lr=lr, betas=(0.9, args.optimizer_beta2), reducer=reducer)
    elif fused_adam_fine_tuning:
        optimizer = FlatAdam(model, lr=lr, betas=(0.9, args.optimizer_beta2),
                             anchor=args.weights_distance_loss or None, lambd=1.0, only=only)
    elif optimizer_kind == "Adam":
        optimizer = torch.optim.Adam(params, lr=lr, betas=(0.9, args.optimizer_beta2))
    elif optimizer_kind == "SGD" and args.fused_optimizer:
        optimizer = FlatSGD(model, lr=lr, anchor=args.weights_distance_loss or None, lambd=1.0, only=only)
    elif optimizer_kind == "SGD":
        optimizer = torch.optim.SGD(params, lr=lr)
    else:
        raise ValueError(f"Unknown optimizer: {optimizer_kind}")
    scheduler = get_lr_scheduler(optimizer=optimizer, epochs=epochs, lr_scheduler_kind=args.lr_scheduler_kind)

    checkpoint_interval = args.checkpoint_interval
    if checkpoint_interval is None:
        checkpoint_interval = 400 if args.dataset == "urban100" else 50

    log = None
    if rank == 0:
        os.makedirs(args.out_dir, exist_ok=True)
        file = open(f"{args.out_dir}/training.csv", "w", newline="", buffering=1)
        log = csv.writer(file)
        log.writerow(["Epoch", "Training Loss"] + (["Estimated Noise Level"] if unsure is not None else [])
                     + (["Estimated Noise Gain"] if unsure_pg else []))

    scheduler_disabled = False
    if args.RESUME is not None:
        ckp = torch.load(args.RESUME, map_location=args.device)
        print("Loading checkpoint from epoch", ckp["epoch"])
        model.load_weights(ckp["params"])
        optimizer.load_state_dict(ckp["optimizer"])
        scheduler.load_state_dict(ckp["scheduler"])
        scheduler_disabled = True                     # as upstream: fixed, explicitly given rate
        assert args.lr is not None
        for group in optimizer.param_groups:
            group["lr"] = args.lr
        if getattr(optimizer, "anchor", None) is not None:    # FlatSGD / FlatAdam with the penalty folded in
            optimizer.anchor.copy_(backbone.flat_params)      # as upstream: the penalty's anchor is the resumed model
        if unsure is not None:
            if "loss_state" not in ckp:
                raise ValueError(f"--sure_unknown_noise: {args.RESUME} holds no loss_state (it was written without the flag)")
            stored, own = ckp["loss_state"].get("noise_state"), unsure.noise_state
            if stored is not None and stored.numel() != own.numel():
                raise ValueError(f"--unsure_noise_model {args.unsure_noise_model}: the loss_state of {args.RESUME} holds "
                                 f"{stored.numel()} floats, this noise model's holds {own.numel()} (4: gaussian, 8: "
                                 "poisson_gaussian); resume with the model the checkpoint was written with")
            unsure.load_state_dict(ckp["loss_state"])         # in place: a captured step reads the buffer's address
    if unsure is not None and os.environ.get("SEI_TRACE_UNSURE_STATE") == "1" and rank == 0:
        eta, m, k = unsure.noise_state[:3].tolist()           # tests: what the first step starts from
        print(f"unsure state at start: eta {eta!r} m {m!r} k {k!r}")
        if unsure_pg:
            gamma, m_gamma = unsure.noise_state[4:6].tolist()
            print(f"unsure gain state at start: gamma {gamma!r} m_gamma {m_gamma!r}")

    def loss_state():
        return None if unsure is None else unsure.state_dict()

    checkpoints_dir = f"{args.out_dir}/checkpoints"

    def checkpoint_name(epoch):
        return f"{checkpoints_dir}/ckp_{epoch:0{len(str(epochs))}}.pt"

    def consolidate():
        """Several GPUs with the sharded optimizer step: every rank brings its float32 weights and Adam moments up to
        date before rank 0 writes them (a collective; a no-op otherwise)."""
        if hasattr(optimizer, "consolidate"):
            optimizer.consolidate()

    consolidate()
    if rank == 0:
        save_training_state(epoch=0, model=model, optimizer=optimizer, scheduler=scheduler,
                            state_path=checkpoint_name(0), loss_state=loss_state())

    # the reference's literal penalty (a deepcopy of the model as it stands here, added to the loss before backward()):
    # every optimizer but FlatSGD and the fine-tuning FlatAdam, whose kernels apply the same penalty and leave its value in
    # `last_penalty`
    fused_penalty = isinstance(optimizer, FlatSGD) or fused_adam_fine_tuning
    weights_distance = None
    if args.weights_distance_loss and not fused_penalty:
        from losses.weights_distance_loss import WeightsDistanceLoss
        weights_distance = WeightsDistanceLoss(pretrained_model=model, lambd=1, device=args.device)

    graphed, early_event = None, None
    trace_step_kind = rank == 0 and os.environ.get("SEI_TRACE_STEP_KIND") == "1"
    for epoch in range(epochs):
        if sampler is not None:
            sampler.set_epoch(epoch)
        loss_sum = torch.zeros((), device=args.device)
        steps = 0
        batches = dataloader if device_cache is None else device_cache.batches(args.batch_size)
        for x, y in batches:
            x, y = x.to(args.device), y.to(args.device)
            used_graph = False
            can_graph = (args.hip_graph and isinstance(optimizer, (FlatAdam, FlatSGD)) and graphs.can_capture(loss)
                         and y.shape[0] == args.batch_size)
            if can_graph:
                if graphed is None:                   # capture once; short last batches run eagerly
                    from graphs import GraphedLossStep
                    early = reducer is not None and os.environ.get("SEI_NO_EARLY_RELEASE") != "1"
                    graphed = GraphedLossStep(loss, model, optimizer,
                                              (args.batch_size, y.shape[1], args.Loss__crop_size, args.Loss__crop_size),
                                              early_release=early,
                                              fuse_optimizer=(reducer is None and args.fuse_optimizer_step
                                                              and isinstance(optimizer, FlatAdam)
                                                              and not fused_adam_fine_tuning))
                    if early and graphed.early_grads is not None:
                        early_event = graphed.early_grads[0]
                        # (a capture after sharded optimizer steps -- the first batches were short -- changes which
                        # slices a rank owns: complete every rank's masters and moments first; a collective, reached by
                        # all ranks at the same step since their shards are equal-length)
                        consolidate()
                        reducer.set_early_range(graphed.early_grads[1:])
                training_loss = graphed(x, y)
                used_graph = True
            else:
                optimizer.zero_grad()
                training_loss = loss(x=x, y=y, model=model)
                if weights_distance is not None:
                    training_loss = training_loss + weights_distance(model)
                training_loss.backward()
            if trace_step_kind:                       # tests: which launch path the first step took
                print("step kind: hipGraph replay" if used_graph else "step kind: eager")
                trace_step_kind = False
            if reducer is not None:
                reducer.reduce_async(early=early_event if used_graph else None,
                                     direct=used_graph and bool(graphed.direct_views))
                if not isinstance(optimizer, FlatAdam):
                    reducer.wait_all()
                    backbone.flat_grads /= world
            optimizer.step()
            loss_sum += training_loss.detach()
            if fused_penalty:
                loss_sum += optimizer.last_penalty            # the logged loss includes the penalty, as upstream
            steps += 1
            if args.max_steps is not None and steps >= args.max_steps:
                break
        if not scheduler_disabled:
            scheduler.step()

        epoch_loss = parallel.all_reduce_mean_scalar(loss_sum / max(steps, 1)).item()
        if (epoch % checkpoint_interval == 0) or (epoch == epochs - 1):
            consolidate()
        if rank == 0:
            stamp = datetime.now().strftime("%Y-%m-%d %H:%M:%S")
            line = f"\t{stamp}\t[{epoch + 1:{len(str(int(epochs)))}d}/{epochs}]\tTraining_Loss: {epoch_loss:.2e}"
            row = [epoch + 1, epoch_loss]
            if unsure is not None:
                estimate = 255 * unsure.estimated_sigma()     # (a sync, once per epoch and outside the step)
                line += f"\tEstimated_Noise_Level: {estimate:.3f}"
                row.append(estimate)
            if unsure_pg:
                gain = unsure.estimated_gain()
                line += f"\tEstimated_Noise_Gain: {gain:.3e}"
                row.append(gain)
            print(line)
            log.writerow(row)
            if (epoch % checkpoint_interval == 0) or (epoch == epochs - 1):
                save_training_state(epoch, model, optimizer, scheduler, checkpoint_name(epoch + 1),
                                    loss_state=loss_state())

    if rank == 0:
        torch.save(model.get_weights(), f"{args.out_dir}/weights.pt")


if __name__ == "__main__":
    main()
