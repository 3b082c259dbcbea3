"""Degradation operators (reference call surface: src/physics/__init__.py).

`get_physics(args, device)` returns an object obeying the deepinv LinearPhysics protocol the
reference's losses, datasets and scripts rely on: A, A_adjoint, __call__ = noise(A(.)), attributes
noise_model (.sigma), task, filter/kernel or rate (CTLikeFilter has neither; BlurDownsampling has rate and sr_filter), and the literally-named "__manager" attribute
exposing randomly_degrade(x, seed). The arithmetic runs in the HIP kernels of libsei_hip.so.
"""
from os.path import exists

import torch

from rng import fork_rng
from ._base import GaussianNoise, LinearPhysics, PoissonGaussianNoise
from .blur import Blur, BlurV2
from .blur_downsampling import BlurDownsampling
from .ct_like_filter import CTLikeFilter
from .downsampling import Downsampling
from .kernels import get_kernel


class BlurKernel:
    """A kernel named in the table, or a path to a torch.save'd 2-D tensor (reference :16-26)."""

    def __init__(self, kernel_path):
        self.kernel_path = kernel_path

    def to_tensor(self, device):
        if exists(self.kernel_path):
            kernel = torch.load(self.kernel_path)
        else:
            kernel = get_kernel(name=self.kernel_path)
        return kernel[None, None].to(device)


class PhysicsManager:
    def __init__(self, blueprint, task, device, noise_level, v2, blur_padding="circular", noise_gain=0.0, sr_kernel=None,
                 sr_phase=0):
        if sr_kernel is not None:            # refused by the flag's name, before any device object exists
            rate = blueprint[Downsampling.__name__]["rate"]
            if task != "sr":
                raise ValueError(f"--sr_kernel names the blur of the super-resolution degradation: it needs --task sr, got "
                                 f"--task {task}")
            if rate is None or int(rate) < 1:
                raise ValueError("--sr_kernel needs --sr_factor, the decimation rate")
            if blur_padding not in BlurDownsampling.PADDINGS:
                raise ValueError(f"--sr_kernel takes --blur_padding {' | '.join(BlurDownsampling.PADDINGS)}: "
                                 f"{blur_padding!r} is refused (with 'valid' the image is not --sr_factor times the measurement)")
            if not 0 <= int(sr_phase) < int(rate):
                raise ValueError(f"--sr_phase must be in [0, --sr_factor): got {sr_phase} at --sr_factor {rate}")
        elif sr_phase:
            raise ValueError("--sr_phase is the sampling phase of --sr_kernel's degradation: give --sr_kernel as well")
        if task == "deblurring":
            kernel = BlurKernel(**blueprint[BlurKernel.__name__]).to_tensor(device)
            # (the FFT operator BlurV2 stands for has no boundary but the circular one)
            if v2 and blur_padding == "circular":
                physics = BlurV2(kernel=kernel)
            else:
                physics = Blur(filter=kernel, padding=blur_padding, device=device)
        elif task == "sr" and sr_kernel is not None:     # blur, then decimate: the blur --task deblurring would build
            kernel = BlurKernel(kernel_path=sr_kernel).to_tensor(device)
            physics = BlurDownsampling(filter=kernel, rate=int(blueprint[Downsampling.__name__]["rate"]),
                                       padding=blur_padding, phase=int(sr_phase), v2=v2)
        elif task == "sr":
            physics = Downsampling(antialias=True, **blueprint[Downsampling.__name__])
        elif task == "invert_a_tomography_like_filter":
            physics = CTLikeFilter()
        else:
            raise ValueError(f"Unknown task: {task}")

        if noise_gain > 0:      # --noise_gain: Poisson-Gaussian measurements, variance (noise_level / 255)^2 + gain * A(x)
            physics.noise_model = PoissonGaussianNoise(sigma=noise_level / 255, gain=noise_gain)
        else:
            physics.noise_model = GaussianNoise(sigma=noise_level / 255)
        self.task = task
        physics.task = task
        setattr(physics, "__manager", self)
        self.physics = physics

    def get_physics(self):
        return self.physics

    def randomly_degrade(self, x, seed):
        """noise(A(x)); with a seed, under a forked RNG seeded with it (reference :65-74)."""
        with fork_rng(enabled=seed is not None):
            if seed is not None:
                torch.manual_seed(seed)
            return self.physics.noise_model(self.physics.A(x))


def get_physics(args, device):
    blueprint = {
        PhysicsManager.__name__: {"task": args.task, "noise_level": args.noise_level, "v2": args.physics_v2,
                                   "blur_padding": getattr(args, "blur_padding", "circular"),
                                   "noise_gain": float(getattr(args, "noise_gain", 0.0) or 0.0),
                                   "sr_kernel": getattr(args, "sr_kernel", None),
                                   "sr_phase": int(getattr(args, "sr_phase", 0) or 0)},
        BlurKernel.__name__: {"kernel_path": args.kernel},
        Downsampling.__name__: {"rate": args.sr_factor, "true_adjoint": args.physics_true_adjoint},
    }
    manager = PhysicsManager(blueprint=blueprint, device=device, **blueprint[PhysicsManager.__name__])
    return manager.get_physics()
