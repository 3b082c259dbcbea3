"""Model factory (reference call surface: src/models/__init__.py).

`get_model(args, physics, device)` returns a `Model` whose forward ignores extra positional arguments,
with `get_backbone() / get_weights() / load_weights()` working on the backbone's state_dict exactly as
the reference's (same keys), so checkpoints interchange.

In scope: kind "Proposed" with architecture "Convolutional" (the in-tree U-Net) or "Transformer" (the
reference's default: deepinv's SwinIR with the arguments at src/models/__init__.py:51-74, rebuilt in
models/swinir.py from the published architecture -- deepinv is not part of the reference tree, parity
unpinned), the trivial "Identity" and "InverseFilter", the bicubic "Upsample" baseline, the classical "TV" baseline
(models/tv.py: proximal gradient on the sei_tv_prox kernel; it needs --tv_lambd, for which the reference has no default
either) and "DeepImagePrior" (models/dip.py: deepinv's untrained ConvDecoder restated, fitted to each measurement by Adam on
the fused sei_dip_* kernels; parity with deepinv unpinned, the float64 restatement in tests/test_dip_baseline_gpu.py is the
pinned truth; --dip_iterations, with the reference's defaults for deblurring and sr) and "PlugAndPlay" (models/pnp.py:
DPIR half-quadratic splitting around the DRUNet of models/drunet.py on the fused sei_drunet_* kernels; the user names the
pretrained weights with --drunet_weights, nothing is fetched; parity with deepinv unpinned, tests/drunet_ref.py is the
pinned truth) and "DiffPIR_DRUNet" (models/diffpir.py: deepinv's DiffPIR restated around the same DRUNet and the same
--drunet_weights, its data step on the fused sei_cg_* conjugate-gradient kernels and its sampling step on
sei_diffpir_sample; --diffpir_iterations, default 100; parity with deepinv unpinned, tests/diffpir_ref.py is the pinned
truth) and "DPS" (models/dps.py: deepinv's DPS restated around the same DRUNet and the same --drunet_weights; every step
differentiates its data term through the denoiser, on DRUNet.forward_taped / DRUNet.vjp -- the sei_drunet_* family with
transposed weights and sei_drunet_conv3x3_masked -- and the sei_dps_* step kernels; --dps_iterations, default 1000; parity
with deepinv unpinned, tests/dps_ref.py is the pinned truth) and "BM3D" (models/bm3d.py: the classical non-learned
deblurring baseline, two regularised inversions each followed by a BM3D stage under coloured noise, restated because the
bm3d package is not here; block matching and the two collaborative filters on the sei_bm3d_* kernels; no weights and no flag;
it needs a physics with a blur kernel; parity with the package unpinned, tests/bm3d_ref.py is the pinned truth) and
"DiffPIR_DiffUNet" (models/diffpir.py's DiffPIRDiffUNet: the same DiffPIR loop, reflect-padded and cropped as the
reference's wrapper does, around the diffusion U-Net of models/diffunet.py -- guided-diffusion's FFHQ-256 network as deepinv's
DiffUNet(large_model=False) builds it -- on the sei_adm_* kernels: GroupNorm, biased 3x3 convolutions, resampling blocks
and global attention; the user names the checkpoint's state dict with --diffunet_weights, nothing is fetched, and without
the flag the kind raises a clear error instead of silently running something else; --diffpir_iterations applies; parity
with deepinv unpinned, tests/diffunet_ref.py is the pinned truth). (One more pretrained network sits outside this
factory: the AlexNet features of the LPIPS metric, metrics.LPIPS, five convolutions whose two small published weight files
the user names to test.py.)
"""
from os import environ

from torch import nn
from torch.nn import Module

from physics import _bands
from physics._ops import SeparableResampleOp, apply_linear
from .bm3d import BM3D
from .convolutional import ConvolutionalModel
from .swinir import SwinIR
from .diffpir import DiffPIR, DiffPIRDiffUNet
from .diffunet import DiffUNet
from .dip import DeepImagePrior
from .dps import DPS
from .drunet import DRUNet
from .pnp import PnPModel
from .tv import TV

_OUT_OF_SCOPE = ("DiffPIR_DiffUNet",)


class Identity(Module):
    def forward(self, y):
        return y


class InverseFilter(Module):
    """The pseudo-inverse of the physics as a "model" (reference :22-28): physics.A_dagger(y) -- least squares by conjugate
    gradients for the blur and the downsampler, the exact inverse filter for CTLikeFilter."""

    def __init__(self, physics):
        super().__init__()
        self.physics = physics

    def forward(self, y):
        return self.physics.A_dagger(y)


class Upsample(Module):
    """The super-resolution baseline (reference src/models/upsample.py): F.interpolate(y, scale_factor=factor,
    mode="bicubic") -- align_corners False, no antialias, no clamp -- as the separable banded resampler over the plain
    bicubic matrices (sei_resample_sepband). No parameters: its state dict is empty."""

    def __init__(self, factor):
        super().__init__()
        if factor is None:
            raise ValueError("model kind 'Upsample' upsamples by the super-resolution factor: give --sr_factor")
        self.factor = factor
        self._op = SeparableResampleOp(lambda n: _bands.plain_bicubic_matrix(n, factor))

    def forward(self, y):
        return apply_linear(self._op, y.contiguous())


class ProposedModel(Module):
    def __init__(self, blueprint, architecture, sampling_rate):
        super().__init__()
        if architecture == "Convolutional":
            self.model = ConvolutionalModel(in_channels=3, upsampling_rate=sampling_rate,
                                            **blueprint[ConvolutionalModel.__name__])
        elif architecture == "Transformer":
            if sampling_rate > 1:
                upsampling_rate, upsampler = sampling_rate, "pixelshuffle"
                if "HOMOGENEOUS_SWINIR" in environ:                 # reference :43-47
                    print("\nUsing homogeneous SwinIR\n")
                    upsampling_rate, upsampler = 1, None
            else:
                upsampling_rate, upsampler = 1, None
            self.model = SwinIR(upscale=upsampling_rate, upsampler=upsampler, img_size=48, patch_size=1, in_chans=3,
                                embed_dim=180, depths=[6, 6, 6, 6, 6, 6], num_heads=[6, 6, 6, 6, 6, 6], window_size=8,
                                mlp_ratio=2, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0,
                                drop_path_rate=0.1, norm_layer=nn.LayerNorm, ape=False, patch_norm=True,
                                use_checkpoint=False, img_range=1.0, resi_connection="1conv", pretrained=None)
        else:
            raise ValueError(f"Unknown model kind: {architecture}")

    def forward(self, y, **kwargs):
        return self.model(y, **kwargs)

    def get_backbone(self):
        return self.model


class Model(Module):
    def __init__(self, blueprint, kind, physics, task, sr_factor, device, noise_level, data_parallel_devices):
        super().__init__()
        sampling_rate = sr_factor if task == "sr" else 1
        if kind == "Proposed":
            self.model = ProposedModel(blueprint=blueprint, sampling_rate=sampling_rate,
                                       **blueprint[ProposedModel.__name__])
        elif kind == "Identity":
            self.model = Identity()
        elif kind == "InverseFilter":
            self.model = InverseFilter(physics=physics)
        elif kind == "Upsample":                              # reference :137-138: by sr_factor whatever the task
            self.model = Upsample(factor=sr_factor)
        elif kind == "TV":                                    # reference :131-132, 210-213: lambd and max_iter from test.py's flags
            self.model = TV(physics=physics, **blueprint[TV.__name__])
        elif kind == "DeepImagePrior":                        # reference :109-114: sr_factor whatever the task
            self.model = DeepImagePrior(physics=physics, sr_factor=sr_factor, **blueprint[DeepImagePrior.__name__])
        elif kind == "PlugAndPlay":                           # reference :115-122: early_stop=True, noise_level / 255
            weights = blueprint[PnPModel.__name__]["drunet_weights"]
            if weights is None:
                raise NotImplementedError("model kind 'PlugAndPlay' runs a pretrained DRUNet and nothing is fetched: name "
                                          "its state dict (KAIR's drunet_color.pth) with --drunet_weights")
            self.model = PnPModel(physics=physics, noise_level_img=noise_level / 255, early_stop=True,
                                  denoiser=DRUNet.from_file(weights, device))
        elif kind == "DiffPIR_DRUNet":                        # reference :125-126 (its wrapper dies on this path: models/diffpir.py)
            weights = blueprint[DiffPIR.__name__]["drunet_weights"]
            if weights is None:
                raise NotImplementedError("model kind 'DiffPIR_DRUNet' runs a pretrained DRUNet and nothing is fetched: name "
                                          "its state dict (KAIR's drunet_color.pth) with --drunet_weights")
            if physics is None:
                raise NotImplementedError("model kind 'DiffPIR_DRUNet' solves its data step with the physics' A and "
                                          "A_adjoint: it cannot run on a folder of measurements without a physics")
            self.model = DiffPIR(physics=physics, denoiser=DRUNet.from_file(weights, device),
                                 max_iter=blueprint[DiffPIR.__name__]["max_iter"])
        elif kind == "DPS":                                   # reference src/models/dps.py: DPSBase(DRUNet, L2())
            weights = blueprint[DPS.__name__]["drunet_weights"]
            if weights is None:
                raise NotImplementedError("model kind 'DPS' runs a pretrained DRUNet and nothing is fetched: name its state "
                                          "dict (KAIR's drunet_color.pth) with --drunet_weights")
            if not callable(getattr(physics, "A", None)) or not callable(getattr(physics, "A_adjoint", None)):
                raise NotImplementedError("model kind 'DPS' differentiates its data term through the physics' A and "
                                          "A_adjoint: a folder of measurements without a physics, or a physics without "
                                          "them, stays outside what this build can run")
            self.model = DPS(physics=physics, denoiser=DRUNet.from_file(weights, device),
                             max_iter=blueprint[DPS.__name__]["max_iter"])
        elif kind == "BM3D":                                  # reference :123-124: sigma_psd = noise_level / 255
            self.model = BM3D(physics=physics, sigma_psd=noise_level / 255)
        elif kind == "DiffPIR_DiffUNet" and blueprint[DiffPIRDiffUNet.__name__]["diffunet_weights"] is not None:
            if physics is None:                               # reference :127-128: DiffPIR(physics, model="DiffUNet")
                raise NotImplementedError("model kind 'DiffPIR_DiffUNet' solves its data step with the physics' A and "
                                          "A_adjoint: it cannot run on a folder of measurements without a physics")
            weights = blueprint[DiffPIRDiffUNet.__name__]["diffunet_weights"]
            self.model = DiffPIRDiffUNet(physics=physics, denoiser=DiffUNet.from_file(weights, device), task=task,
                                         max_iter=blueprint[DiffPIRDiffUNet.__name__]["max_iter"])
        elif kind in _OUT_OF_SCOPE:                           # the no-weights path of DiffPIR_DiffUNet
            raise NotImplementedError(f"model kind {kind!r} is an evaluation baseline outside the training "
                                      "hot path this build implements unless its pretrained diffusion U-Net is named: "
                                      "nothing is fetched, give the state dict of the FFHQ checkpoint that deepinv's "
                                      "DiffUNet(large_model=False) loads with --diffunet_weights")
        else:
            raise ValueError(f"Unknown model kind: {kind}")
        if data_parallel_devices is not None:
            # reference :142-145,178-182: nn.DataParallel over these device ids, re-replicating the weights on
            # every forward. Here one process per GPU owns a replica; the same devices are used by:
            n = len(data_parallel_devices)
            ids = ",".join(data_parallel_devices)
            raise NotImplementedError(
                f"--data_parallel_devices {ids}: single-process nn.DataParallel is replaced by one process per "
                f"GPU with an RCCL gradient all-reduce (parallel.py). Equivalent launch on the same devices:\n"
                f"  HIP_VISIBLE_DEVICES={ids} python -m torch.distributed.run --nnodes=1 --nproc-per-node {n} "
                f"--master-addr 127.0.0.1 train.py <the same flags without --data_parallel_devices> "
                f"--batch_size <batch_size / {n}>")

    def forward(self, x, *args, **kwargs):
        """Extra positional arguments are ignored, as upstream (:148-149); keyword arguments (the SwinIR backbone's
        injected stochastic-depth masks) go to the backbone."""
        return self.model(x, **kwargs)

    def get_backbone(self):
        model = self.model
        return model.get_backbone() if isinstance(model, ProposedModel) else model

    def get_weights(self):
        return self.get_backbone().state_dict()

    def load_weights(self, state_dict):
        self.get_backbone().load_state_dict(state_dict)


def _dip_iterations(args):
    """--dip_iterations, else the reference's defaults (:194-205): 4000 for deblurring with a Gaussian kernel, 1000 for
    other deblurring and for sr. For any other task the reference leaves the name unbound."""
    given = getattr(args, "dip_iterations", None)
    if given is not None:
        return given
    if args.task == "deblurring":
        return 4000 if "Gaussian" in (args.kernel or "") else 1000
    if args.task == "sr":
        return 1000
    raise ValueError(f"model kind 'DeepImagePrior' has no default iteration count for --task {args.task}: "
                     "give --dip_iterations")


def get_model(args, physics, device):
    data_parallel_devices = (args.data_parallel_devices.split(",")
                             if args.data_parallel_devices is not None else None)
    blueprint = {
        ConvolutionalModel.__name__: {
            "residual": args.ConvolutionalModel__residual,
            "inner_residual": args.ConvolutionalModel__inner_residual,
            "num_conv_blocks": args.ConvolutionalModel__num_conv_blocks,
            "inout_convs": args.ConvolutionalModel__inout_convs,
            "hidden_channels": args.ConvolutionalModel__hidden_channels,
            "scales": args.ConvolutionalModel__scales,
        },
        Model.__name__: {
            "task": args.task,
            "sr_factor": args.sr_factor,
            "noise_level": args.noise_level,
            "kind": args.model_kind,
        },
        ProposedModel.__name__: {"architecture": args.ProposedModel__architecture},
        # (train.py's parser has neither flag; the reference passes a missing --tv_lambd on as None and dies in deepinv,
        # TV raises NotImplementedError naming the flag)
        DeepImagePrior.__name__: {"iterations": _dip_iterations(args) if args.model_kind == "DeepImagePrior" else None},
        PnPModel.__name__: {"drunet_weights": getattr(args, "drunet_weights", None)},
        DiffPIR.__name__: {"drunet_weights": getattr(args, "drunet_weights", None),
                           "max_iter": 100 if getattr(args, "diffpir_iterations", None) is None
                           else args.diffpir_iterations},
        DiffPIRDiffUNet.__name__: {"diffunet_weights": getattr(args, "diffunet_weights", None),
                                   "max_iter": 100 if getattr(args, "diffpir_iterations", None) is None
                                   else args.diffpir_iterations},
        DPS.__name__: {"drunet_weights": getattr(args, "drunet_weights", None),
                       "max_iter": 1000 if getattr(args, "dps_iterations", None) is None else args.dps_iterations},
        TV.__name__: {"lambd": getattr(args, "tv_lambd", None), "max_iter": getattr(args, "tv_max_iter", None) or 300},
    }
    return Model(blueprint=blueprint, physics=physics, device=device,
                 data_parallel_devices=data_parallel_devices, **blueprint[Model.__name__])
