#!/usr/bin/env python3
"""Evaluation driver with the reference's command line (reference: demo/test.py).

    python test.py --device cuda --task deblurring --kernel Gaussian_R2 --ProposedModel__architecture Convolutional \
        --dataset div2k --GroundTruthDataset__datasets_dir ./datasets --weights runs/x/weights.pt

For every test pair: x_hat = model(y) under no_grad (the same HIP forward as training, any image size; with --task
invert_a_tomography_like_filter up to the extents sei_circ_filter_sep holds in LDS, about 560 per axis), then
quantise to 8 bits and clamp x, y, x_hat (reference :140-148), PSNR on the luma channel (src/metrics.py), and
the reference's summary lines. In scope: the Proposed model family and the Identity / InverseFilter / bicubic Upsample
kinds, `--dataset div2k | single_image | synthetic` or a directory of PNG measurements, `--save_images`, `--save_psf`,
`--indices`, `--print_all_metrics`, `--noise2inverse` (src/noise2inverse.py's sliced evaluation around the same
backbone), `--r2r`, and the classical baseline `--model_kind TV --tv_lambd L [--tv_max_iter N]` (models/tv.py: proximal
gradient on sei_tv_prox; without --tv_lambd it raises, the reference has no default either) and `--model_kind DeepImagePrior
[--dip_iterations N]` (models/dip.py: an untrained decoder fitted to every measurement by Adam on the sei_dip_* kernels; its
forward needs no autograd, so the reference's `dip` switch around no_grad has nothing to do here) and `--model_kind
PlugAndPlay --drunet_weights FILE` (models/pnp.py: DPIR half-quadratic splitting, eight calls of the DRUNet of models/drunet.py
on the sei_drunet_* kernels per image; FILE is the state dict of KAIR's drunet_color.pth, never fetched: without the flag it
raises and names it) and `--model_kind DiffPIR_DRUNet --drunet_weights FILE [--diffpir_iterations N]` (models/diffpir.py:
deepinv's DiffPIR restated around the same DRUNet, N = 100 denoiser calls per image by default and between them the data
step's conjugate gradients on the fused sei_cg_* kernels and the sampling step on sei_diffpir_sample; its noise comes from
torch's generator, seeded above like everything else) and `--model_kind DPS --drunet_weights FILE [--dps_iterations N]`
(models/dps.py: deepinv's DPS restated around the same DRUNet; every one of its N = 1000 default steps is a denoiser forward
and a vector-Jacobian product through it, DRUNet.forward_taped / DRUNet.vjp on the sei_drunet_* kernels, with the step itself
on the sei_dps_* kernels: the heaviest path of this driver). `--ssim` (build-side addition) computes the luma SSIM (metrics.ssim_fn, sei_ssim_luma) for the
`SSIM:`, `SSIM std:` and `METRICS_i` lines; without it they print nan, as before. `--lpips_backbone FILE --lpips_linear FILE`
(build-side addition; both or neither) name a torchvision AlexNet state dict and the LPIPS v0.1 `alex` linear layers: the
`LPIPS:`, `LPIPS std:` and `LIPS:` fields then carry metrics.lpips_fn's values (the sei_lpips_* kernels); without them they
print nan (the pretrained weights are not part of this build and are never fetched). `--model_kind BM3D` (models/bm3d.py: the
classical deblurring baseline, restated because the bm3d package is not here; two regularised inversions in torch.fft, each
followed by block matching and a collaborative filter on the sei_bm3d_* kernels; no weights and no flag of its own; it needs a
physics with a blur kernel, so --task sr and a folder of measurements are refused). `--model_kind DiffPIR_DiffUNet
--diffunet_weights FILE [--diffpir_iterations N]` (models/diffpir.py's DiffPIRDiffUNet around models/diffunet.py: the same
DiffPIR loop on the reflect-padded measurement, cropped afterwards as the reference's wrapper does, with the diffusion U-Net
of deepinv's DiffUNet(large_model=False) on the sei_adm_* kernels as its denoiser; FILE is the state dict of the FFHQ
checkpoint deepinv fetches, supplied by the user and never fetched here; without the flag the kind raises and names it).
`--bootstrap N [--bootstrap_batch B] [--bootstrap_maps]` (build-side addition; bootstrap.py: the equivariant bootstrap of
Tachella and Pereyra, restated from the paper) estimates every image's error from its measurement alone, with or without
ground truth: N times the estimate is zoomed out by a random rate about a random centre (the EI loss's draws), measured again
through the physics with fresh noise and reconstructed again, B replicas per model call (default 8; a model kind that takes
one image at a time needs 1), on the sei_boot_* kernels; the replicas go through the plain model call, also under
--noise2inverse and --r2r. The bootstrap of image i draws under a forked generator seeded with i, so every other line of
the output is what it is without the flag. `BOOTSTRAP_i: EST_PSNR, EST_PSNR_Q90` per image under
--print_all_metrics, and `EST_N`, `EST_PSNR`, `EST_PSNR std`, `EST_PSNR_Q90` at the end; with a folder of measurements the
physics of --task / --kernel / --sr_factor / --noise_level is built for the bootstrap alone. --bootstrap_maps (needs --out_dir)
writes error_maps/NAME.npy (float32 root-mean-square error per pixel) and NAME.png (the same over its own maximum): a
qualitative picture of where the errors sit. Calibration of EST_PSNR against the true PSNR is not shown in this build (no
trained weights); on a dataset with ground truth both are printed side by side.
`--estimate_noise gaussian | poisson_gaussian` (build-side addition; noise_estimation.py, the sei_noise_* kernels: the
project's own estimator) reads the noise levels off the measurements themselves: `NOISE_i: SIGMA_255, ETA, GAIN`
per image under --print_all_metrics and `EST_NOISE_N`, `EST_SIGMA_255`, `EST_ETA`, `EST_GAIN` at the end, pooled over every
processed measurement through one accumulated histogram (variance = ETA + GAIN * signal; SIGMA_255 is the Gaussian level on
--noise_level's scale). It draws no random numbers: every other line is what it is without the flag. With a folder of
measurements and --bootstrap, the whole folder is estimated first and the bootstrap's physics gets the estimated level
(gaussian: sigma; poisson_gaussian: sqrt(eta) and the gain, or sigma with a notice when the two-level fit did not hold)
in place of --noise_level / --noise_gain, which nobody knows for measured data; one line says which levels it used. On a
dataset with ground truth the flag only prints: the synthetic physics keeps its flags.
`--tile T [--tile_overlap V] [--tile_batch B] [--tile_window feather | uniform | crop]` (build-side addition; tiling.py, the
sei_tile_* kernels) reconstructs every image from overlapping T x T tiles (T a multiple of 16 up to 2048,
2 V <= T, default V = 32), B tiles per model call, blended under the window: frames of any size at the memory of a tile.
Every model call of this driver then goes through one tiling.TiledModel: the plain path, the --noise2inverse backbone, the
--r2r loop and the bootstrap's replicas. Feed-forward kinds only (Proposed, Identity, Upsample); for the networks of this
build tiling is an approximation whose seams the overlap hides, not the whole-image result. Without the flag every call and
every printed line is what it was.
"""
import os
import sys
from argparse import BooleanOptionalAction
from os.path import basename, dirname, isdir

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "scale-equivariant-imaging_amd"))

from datasets import get_dataset  # noqa: E402
from datasets._io import read_image  # noqa: E402
from metrics import LPIPS, compute_metrics  # noqa: E402
from models import get_model  # noqa: E402
from physics import get_physics  # noqa: E402
from rng import fork_rng  # noqa: E402
from settings import DefaultArgParser  # noqa: E402
from training import get_weights  # noqa: E402


def build_parser():
    parser = DefaultArgParser()
    flag = parser.add_argument
    flag("--weights", type=str)
    flag("--save_images", action="store_true")
    flag("--indices", type=str, default=None)
    flag("--out_dir", type=str, default=None)
    flag("--save_psf", action="store_true")
    flag("--dip_iterations", type=int, default=None)
    flag("--noise2inverse", action="store_true")
    flag("--print_all_metrics", action="store_true")
    flag("--r2r", action="store_true")
    flag("--r2r_itercount", type=int, default=1)
    flag("--tv_lambd", type=float, default=None)
    flag("--tv_max_iter", type=int, default=300)
    flag("--GroundTruthDataset__split", type=str, default="val")
    flag("--SyntheticDataset__deterministic_measurements", action=BooleanOptionalAction, default=True)
    flag("--memoize_gt", action=BooleanOptionalAction, default=False)
    flag("--compute_dtype", choices=["f32", "bf16", "bf16x3"], default="f32")          # build-side addition
    flag("--ssim", action="store_true")                                                  # build-side addition
    flag("--lpips_backbone", type=str, default=None, metavar="FILE")                     # build-side addition
    flag("--lpips_linear", type=str, default=None, metavar="FILE")                       # build-side addition
    flag("--drunet_weights", type=str, default=None, metavar="FILE")                     # build-side addition
    flag("--diffunet_weights", type=str, default=None, metavar="FILE")                   # build-side addition
    flag("--diffpir_iterations", type=int, default=100)                                  # build-side addition
    flag("--dps_iterations", type=int, default=1000)                                     # build-side addition
    flag("--bootstrap", type=int, default=0, metavar="N")                                # build-side addition
    flag("--bootstrap_batch", type=int, default=8, metavar="B")                          # build-side addition
    flag("--bootstrap_maps", action="store_true")                                        # build-side addition
    flag("--estimate_noise", choices=["gaussian", "poisson_gaussian"], default=None)     # build-side addition
    flag("--tile", type=int, default=0, metavar="T")                                     # build-side addition
    flag("--tile_overlap", type=int, default=32, metavar="V")                            # build-side addition
    flag("--tile_batch", type=int, default=8, metavar="B")                               # build-side addition
    flag("--tile_window", choices=["feather", "uniform", "crop"], default="feather")     # build-side addition
    return parser


def parse_args(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if (args.lpips_backbone is None) != (args.lpips_linear is None):
        given, other = ("--lpips_backbone", "--lpips_linear") if args.lpips_linear is None else \
            ("--lpips_linear", "--lpips_backbone")
        parser.error(f"{given} needs {other} as well: LPIPS takes both weight files or neither")
    if args.bootstrap < 0 or args.bootstrap_batch < 1:
        parser.error("--bootstrap takes a replica count >= 0 and --bootstrap_batch a chunk size >= 1")
    if args.bootstrap_maps and args.out_dir is None:
        parser.error("--bootstrap_maps needs --out_dir")
    if args.tile < 0 or args.tile % 16 != 0 or args.tile > 2048:
        parser.error("--tile takes a multiple of 16 up to 2048 (neither SwinIR's window of 8 nor the U-Net's 2^4 then pads "
                     "a full tile; 0 switches tiling off)")
    if args.tile_overlap < 0 or (args.tile and 2 * args.tile_overlap > args.tile):
        parser.error("--tile_overlap takes an overlap V >= 0 with 2 V <= --tile")
    if args.tile_batch < 1:
        parser.error("--tile_batch takes a chunk size >= 1")
    if args.tile and args.model_kind not in TILED_KINDS:
        parser.error(f"--tile runs feed-forward model kinds only ({', '.join(TILED_KINDS)}): --model_kind {args.model_kind} "
                     "carries the physics at the whole image's extents inside the model, and tiling it would be a different "
                     "algorithm")
    if args.tile and tile_scale(args) * args.tile > 2048:
        parser.error(f"--tile times the super-resolution factor {tile_scale(args)} must stay within 2048 output pixels")
    return args


TILED_KINDS = ("Proposed", "Identity", "Upsample")


def tile_scale(args):
    """The integer by which the model multiplies the extents of its input: the physics' rate for a Proposed SR model,
    --sr_factor for the bicubic Upsample kind whatever the task, 1 otherwise (also for the homogeneous SwinIR of
    models/__init__.py, which maps measurements already brought to the ground truth's size)."""
    if args.model_kind == "Proposed" and args.ProposedModel__architecture == "Transformer" and "HOMOGENEOUS_SWINIR" in os.environ:
        return 1
    if args.model_kind == "Upsample" or (args.model_kind == "Proposed" and args.task == "sr"):
        return int(args.sr_factor or 1)
    return 1


def quantize_and_clamp(im):
    """8-bit quantisation, then clamping (reference :141-145)."""
    return ((im * 255.0).round() / 255.0).clamp(0.0, 1.0)


def save_image(im, path):
    """(1, C, H, W) or (C, H, W) in [0, 1] -> PNG (torchvision.utils.save_image for one image: x255 + 0.5, uint8)."""
    from PIL import Image
    im = im.detach()
    if im.dim() == 4:
        im = im[0]
    if im.dim() == 2:
        im = im[None]
    a = im.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()
    Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a).save(path)


def main(argv=None):
    torch.manual_seed(0)
    np.random.seed(0)
    args = parse_args(argv)
    from models import _ops as model_ops
    model_ops.set_compute_dtype(args.compute_dtype)

    physics = None if isdir(args.dataset) else get_physics(args, device=args.device)
    model = get_model(args=args, physics=physics, device=args.device)
    model.to(args.device)
    model.eval()
    if args.weights is not None:
        model.load_weights(get_weights(args.weights, args.device))

    forward = model                                           # every model call below goes through it
    if args.tile:
        from tiling import TiledModel
        forward = TiledModel(model, tile=args.tile, overlap=args.tile_overlap, batch=args.tile_batch,
                             scale=tile_scale(args), window=args.tile_window)

    bootstrap = None
    if args.bootstrap:                                        # (a folder of measurements: the physics is built for it alone)
        from bootstrap import EquivariantBootstrap
        boot_physics = physics if physics is not None else get_physics(args, device=args.device)
        bootstrap = EquivariantBootstrap(boot_physics, lambda v: forward(v.contiguous()), samples=args.bootstrap,
                                         batch=args.bootstrap_batch)
    est_list, q90_list = [], []

    lpips_net = None
    if args.lpips_backbone is not None:
        lpips_net = LPIPS.from_files(args.lpips_backbone, args.lpips_linear, device=args.device)

    basename_table = {}
    if isdir(args.dataset):                                   # a folder of measurements, no ground truth
        from glob import glob
        dataset = []
        for i, f in enumerate(glob(os.path.join(args.dataset, "*.png"))):
            y = read_image(f).to(args.device).float() / 255.0
            dataset.append((None, y[:3, :, :]))               # discard the alpha channel if it exists
            basename_table[i] = basename(f)
    else:
        dataset = get_dataset(args=args, purpose="test", physics=physics, device=args.device, _HOTFIX=False)

    noise_pooled, noise_count = None, 0
    if args.estimate_noise is not None:
        from noise_estimation import NoiseEstimator, bootstrap_levels
        from physics import GaussianNoise, PoissonGaussianNoise
        noise_pooled, noise_single = NoiseEstimator(args.device), NoiseEstimator(args.device)
        if bootstrap is not None and physics is None:         # measured data: nobody knows --noise_level / --noise_gain
            for _, y in dataset:
                noise_single.add(y)
            sigma, gain, notice = bootstrap_levels(noise_single.estimate(), args.estimate_noise)
            if notice is not None:
                print(f"BOOTSTRAP_NOISE: {notice}")
            boot_physics.noise_model = PoissonGaussianNoise(sigma=sigma, gain=gain) if gain > 0 else \
                GaussianNoise(sigma=sigma)
            print(f"BOOTSTRAP_NOISE: the bootstrap measures again with SIGMA_255: {255 * sigma:.3f}, GAIN: {gain:.5f} "
                  f"(--estimate_noise {args.estimate_noise} over {len(dataset)} measurements)")

    if args.save_psf:
        assert args.out_dir is not None
        assert physics.task == "deblurring"
        kernel = physics.filter
        assert kernel.dim() == 4
        kernel = kernel.squeeze(0).squeeze(0)
        os.makedirs(args.out_dir, exist_ok=True)
        save_image((kernel / kernel.max()).float(), os.path.join(args.out_dir, "psf.png"))

    indices = range(len(dataset)) if args.indices is None else (int(i) for i in args.indices.split(","))
    psnr_list, ssim_list, lpips_list = [], [], []
    for i in indices:
        x, y = dataset[i]
        x = x.unsqueeze(0) if x is not None else None
        y = y.unsqueeze(0)
        if noise_pooled is not None:
            noise_pooled.add(y)
            noise_count += 1
            if args.print_all_metrics:
                one = noise_single.reset().add(y).estimate()
                print(f"NOISE_{i}: SIGMA_255: {one['sigma_255']:.3f}, ETA: {one['eta']:.3e}, GAIN: {one['gain']:.5f}")
        with torch.no_grad():
            if args.noise2inverse:                            # reference demo/test.py:116-126
                from noise2inverse import Noise2InverseModel
                if physics.task != "deblurring" and not hasattr(physics, "A_dagger"):
                    raise NotImplementedError("--noise2inverse needs physics.A_dagger outside deblurring")
                wrapped = Noise2InverseModel(backbone=lambda v: forward(v.contiguous()), task=physics.task,
                                             physics_filter=getattr(physics, "filter", None),
                                             degradation_inverse_fn=getattr(physics, "A_dagger", None))
                x_hat = wrapped(y)
            elif args.r2r:                                    # :127-134
                x_hat = torch.zeros_like(x)
                for _ in range(args.r2r_itercount):
                    pert = torch.randn_like(y) * physics.noise_model.sigma
                    x_hat += forward((y + 0.5 * pert).contiguous())
                x_hat /= args.r2r_itercount
            else:
                x_hat = forward(y.contiguous())
        if bootstrap is not None:
            with fork_rng(enabled=True):                      # its draws leave the stream of the images that follow alone
                torch.manual_seed(i)
                boot = bootstrap(y.contiguous(), x_hat=x_hat)
            est_list.append(boot["est_psnr"])
            q90_list.append(boot["est_psnr_q90"])
            if args.print_all_metrics:
                print(f"BOOTSTRAP_{i}: EST_PSNR: {boot['est_psnr']:.2f}, EST_PSNR_Q90: {boot['est_psnr_q90']:.2f}")
            if args.bootstrap_maps:
                rmse = boot["rmse_map"]
                stem = os.path.join(args.out_dir, "error_maps", os.path.splitext(basename_table.get(i, f"{i}.png"))[0])
                os.makedirs(dirname(stem), exist_ok=True)
                np.save(stem + ".npy", rmse.cpu().numpy())
                save_image(rmse / rmse.max().clamp_min(1e-30), stem + ".png")
        x = quantize_and_clamp(x) if x is not None else None
        y = quantize_and_clamp(y)
        x_hat = quantize_and_clamp(x_hat)
        if x is not None:
            psnr_val, ssim_val, lpips_val = compute_metrics(x.squeeze(0), x_hat.squeeze(0), ssim=args.ssim,
                                                            lpips=lpips_net)
            psnr_list.append(psnr_val)
            ssim_list.append(ssim_val)
            lpips_list.append(lpips_val)
            if args.print_all_metrics:
                print(f"METRICS_{i}: PSNR: {psnr_val:.2f}, SSIM: {ssim_val:.4f}, LIPS: {lpips_val:.4f}")
        if args.save_images:
            assert args.out_dir is not None
            entry = basename_table.get(i, f"{i}.png")
            for folder, im in (("ground_truth", x), ("predictors", y), ("estimates", x_hat)):
                if im is None:
                    continue
                path = os.path.join(args.out_dir, folder, entry)
                os.makedirs(dirname(path), exist_ok=True)
                save_image(im, path)

    n = len(psnr_list)
    if n != 0:
        print(f"N: {n}")
        print(f"PSNR: {np.mean(psnr_list):.2f}")
        print(f"PSNR std: {np.std(psnr_list):.2f}")
        print(f"SSIM: {np.mean(ssim_list):.4f}")
        print(f"SSIM std: {np.std(ssim_list):.4f}")
        print(f"LPIPS: {np.mean(lpips_list):.4f}")
        print(f"LPIPS std: {np.std(lpips_list):.4f}")
    if est_list:
        print(f"EST_N: {len(est_list)}")
        print(f"EST_PSNR: {np.mean(est_list):.2f}")
        print(f"EST_PSNR std: {np.std(est_list):.2f}")
        print(f"EST_PSNR_Q90: {np.mean(q90_list):.2f}")
    if noise_count:
        pooled = noise_pooled.estimate()
        print(f"EST_NOISE_N: {noise_count}")
        print(f"EST_SIGMA_255: {pooled['sigma_255']:.3f}")
        print(f"EST_ETA: {pooled['eta']:.3e}")
        print(f"EST_GAIN: {pooled['gain']:.5f}")
    return psnr_list


if __name__ == "__main__":
    main()
