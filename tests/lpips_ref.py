"""Shared by tests/test_lpips.py and tests/test_lpips_gpu.py: synthetic LPIPS weights in the two published file layouts,
and a restatement of LPIPS v0.1 (AlexNet) written here from the definition with F.conv2d / F.max_pool2d, in any dtype
(float64: the truth the tests pin; float32: the CPU chain the kernels' feature maps are measured against). Nothing here
imports metrics.py."""
import math

import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# torchvision AlexNet features: (Sequential index, Cin, Cout, kernel, stride, zero pad, followed by maxpool(3, 2))
LAYERS = ((0, 3, 64, 11, 4, 2, True), (3, 64, 192, 5, 1, 2, True), (6, 192, 384, 3, 1, 1, False),
          (8, 384, 256, 3, 1, 1, False), (10, 256, 256, 3, 1, 1, False))


def synthetic_state_dicts(seed=1234):
    """(backbone, linear): conv weights randn * sqrt(2 / (Cin k k)), biases randn * 0.1, linear weights rand; the backbone
    also carries a classifier entry that a loader has to ignore."""
    g = torch.Generator().manual_seed(seed)
    backbone, linear = {}, {}
    for l, (idx, cin, cout, k, _, _, _) in enumerate(LAYERS):
        backbone[f"features.{idx}.weight"] = torch.randn((cout, cin, k, k), generator=g) * math.sqrt(2.0 / (cin * k * k))
        backbone[f"features.{idx}.bias"] = torch.randn((cout,), generator=g) * 0.1
        linear[f"lin{l}.model.1.weight"] = torch.rand((1, cout, 1, 1), generator=g)
    backbone["classifier.1.weight"] = torch.randn((8, 16), generator=g)
    backbone["classifier.1.bias"] = torch.randn((8,), generator=g)
    return backbone, linear


def write_files(folder, backbone, linear, prefix=""):
    """torch.save both dicts (the linear one with `prefix` in front of every key) -> (backbone path, linear path)."""
    pb, pl = str(folder / "alexnet.pth"), str(folder / "lpips_alex.pth")
    torch.save(backbone, pb)
    torch.save({prefix + k: v for k, v in linear.items()}, pl)
    return pb, pl


def features_ref(backbone, x, dtype=torch.float64):
    """(B, 3, H, W) in [0, 1] -> the five ReLU outputs, in `dtype` on the CPU."""
    x = x.to("cpu", dtype)
    shift = torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    h = ((2 * x - 1) - shift) / scale                       # the zero padding of conv1 pads THIS, not x
    out = []
    for idx, _, _, _, stride, pad, pool in LAYERS:
        w, b = backbone[f"features.{idx}.weight"].to(dtype), backbone[f"features.{idx}.bias"].to(dtype)
        h = F.relu(F.conv2d(h, w, b, stride=stride, padding=pad))
        out.append(h)
        if pool:
            h = F.max_pool2d(h, kernel_size=3, stride=2)     # floor mode, no padding
    return out


def lpips_ref(backbone, linear, a, b, dtype=torch.float64):
    """(B, 3, H, W) pairs -> (B,) in `dtype`."""
    total = torch.zeros(a.shape[0], dtype=dtype)
    for l, (fa, fb) in enumerate(zip(features_ref(backbone, a, dtype), features_ref(backbone, b, dtype))):
        na = fa / (torch.sqrt((fa * fa).sum(dim=1, keepdim=True)) + 1e-10)
        nb = fb / (torch.sqrt((fb * fb).sum(dim=1, keepdim=True)) + 1e-10)
        w = linear[f"lin{l}.model.1.weight"].to(dtype)
        total = total + (w * (na - nb) ** 2).sum(dim=1).mean(dim=(-2, -1))
    return total


def pair(B, H, W, s, seed):
    """x = rand, x_hat = clamp(x + s randn, 0, 1), float32."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, 3, H, W), generator=g)
    x_hat = (x + s * torch.randn((B, 3, H, W), generator=g)).clamp(0, 1)
    return x_hat, x
