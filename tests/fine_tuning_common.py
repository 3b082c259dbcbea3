"""Small flat-bucket modules and the float64 restatement shared by tests/test_fine_tuning.py (CPU) and
tests/test_fine_tuning_gpu.py: the four-parameter module of the g17 fixture, a two-parameter module for the loop shapes of
sei_sgd_fused, and a nested one whose names end in `model.model.conv_last.*` as SwinIR's do."""
import numpy as np
import torch

from models._flat import FlatParameterBucket

G17_SHAPES = {"w0": (5, 3, 3, 3), "b0": (1,), "w1": (64, 32, 1, 1), "b1": (65,)}


class Bucket(FlatParameterBucket, torch.nn.Module):
    """Parameters named and shaped by `shapes`, values from `values` (numpy arrays or tensors) or seeded normals."""

    def __init__(self, shapes, values=None, seed=0):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        for name, shape in shapes.items():
            v = torch.randn(shape, generator=gen) if values is None else torch.as_tensor(np.asarray(values[name]))
            setattr(self, name, torch.nn.Parameter(v.float().clone()))
        self._init_bucket()
        self.flatten_parameters()


class _Tail(FlatParameterBucket, torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.body = torch.nn.Conv2d(3, 20, 3)                 # 540 + 20
        self.mix = torch.nn.Conv2d(32, 64, 1)                 # a 1x1 weight: goes last in the bucket
        self.conv_last = torch.nn.Conv2d(20, 3, 3)            # 540 + 3, like SwinIR's tail
        self._init_bucket()
        self.flatten_parameters()


class _Mid(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.model = _Tail()


class Nested(torch.nn.Module):
    """Parameter names `model.model.<layer>.*` around a flat-bucket backbone, as the project's SwinIR wrapper has them."""

    def __init__(self, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.model = _Mid()

    def get_backbone(self):
        return self.model.model


def g17_values(g, prefix):
    return {name: g[f"{prefix}.{name}"] for name in G17_SHAPES}


def per_element(model, per_name, dtype=torch.float64):
    """A bucket-long CPU tensor holding per_name[name] at each parameter's range and zero in the padding."""
    backbone = model.get_backbone() if hasattr(model, "get_backbone") else model
    out = torch.zeros(backbone.flat_params.numel(), dtype=dtype)
    for name, p in model.named_parameters():
        v = torch.as_tensor(np.asarray(per_name[name])) if not isinstance(per_name[name], torch.Tensor) else per_name[name]
        out[p._sei_bucket_offset:p._sei_bucket_offset + p.numel()] = v.detach().cpu().reshape(-1).to(dtype)
    return out


def coefficients(model, lambd=1.0):
    """lambd / (K n_k) per element of the bucket in float64 (zero in the padding), from the names alone."""
    named = list(model.named_parameters())
    return per_element(model, {n: torch.full((p.numel(),), lambd / (len(named) * p.numel()), dtype=torch.float64)
                               for n, p in named})


def padding_mask(model):
    backbone = model.get_backbone() if hasattr(model, "get_backbone") else model
    mask = torch.ones(backbone.flat_params.numel(), dtype=torch.bool)
    for p in model.parameters():
        mask[p._sei_bucket_offset:p._sei_bucket_offset + p.numel()] = False
    return mask


def restated_step(p, g, a, c, lr, ranges=None):
    """The fine-tuning step in float64 on bucket-long tensors: (updated p, penalty from the p before the update);
    `ranges`: the (lo, hi) slices that move (everything when None). The penalty is over the whole bucket either way."""
    d = p - a
    penalty = float((c * d * d).sum())
    new = p - lr * (g + 2 * c * d)
    if ranges is not None:
        keep = torch.ones_like(p, dtype=torch.bool)
        for lo, hi in ranges:
            keep[lo:hi] = False
        new = torch.where(keep, p, new)
    return new, penalty


def penalty_bar(ref32, ref64):
    """The bar of the issue for a penalty value: twice the reference's own float32 error, at least 1e-6 relative."""
    return max(2 * abs(float(ref32) - float(ref64)), 1e-6 * abs(float(ref64)))
