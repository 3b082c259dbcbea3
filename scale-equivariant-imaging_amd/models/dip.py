"""The Deep Image Prior baseline (reference: src/models/dip.py, src/models/__init__.py:109-114, 194-208): an untrained
convolutional decoder G fitted to ONE measurement y by `iterations` Adam steps on mean((A(G(z)) - y)^2), z a fixed random
code. deepinv is not part of the reference tree, so this restates deepinv v0.2.0's `ConvDecoder` and `DeepImagePrior` from
their published definition; parity with deepinv itself is UNPINNED. The pinned truth is the float64 torch restatement in
tests/test_dip_baseline_gpu.py.

The decoder, ConvDecoder(img_shape=(C_out, H, W), in_size=[16, 16], layers=7, channels=32). Stage extents in Python doubles:

    sx = (H / in_size[0]) ** (1 / (layers - 1));  sy likewise with W
    hidden = [(ceil(sx**n * in_size[0]), ceil(sy**n * in_size[1])) for n in 1 .. layers - 2] + [(H, W)]

for i in 0 .. layers - 2: Upsample(size=hidden[i], "nearest"), Conv2d(ch, ch, 3, padding 1), ReLU, BatchNorm2d(ch); then one
more Conv3x3, ReLU, BatchNorm at the final size and Conv2d(ch, C_out, 1). BatchNorm is always in training mode (the backbone
is built inside forward and never put in eval): batch statistics over the H W pixels of the single item, biased variance,
eps 1e-5. Extents may shrink from one stage to the next (a 12 x 20 image from a 16 x 16 code).

Everything on the GPU is csrc/dip_kernels.hip (float32, channels-last, 32 channels): one fused launch per stage that applies
the previous BatchNorm and the nearest index on load, so neither the normalised nor the upsampled tensor exists; a gather
for the upsample's adjoint; two-stage reductions without atomics. The data-fit term is sei_mse_loss, A and its transpose are
the physics operator's own kernel (physics._ops), the update is sei_dip_adam: sei_adam_fused's arithmetic with the step's
scalars read from the device array that sei_adam_scalars_to_device fills (sei_adam_fused takes them as launch arguments,
which a captured launch would freeze at step 1). One iteration is a fixed chain of launches without host synchronisation:
after a short eager warm-up it is captured once and replayed (`graph=False` keeps the eager loop; both give the same bits).

Deliberate choices:
- Batch 1 only (ValueError otherwise); test.py never sends another.
- The decoder is initialised on the CPU with torch's own modules in module order, i.e. torch's default initialisation from
  the CPU generator, as the reference's construct-then-.to(device) does; z comes from the device generator.
- No state survives a forward: the state dict is empty.
"""
import math

import numpy as np
import torch
from torch import nn
from torch.nn import Module

import _native as N

BN_EPS = 1e-5
WARMUP = 3


def decoder_sizes(img_hw, in_size=(16, 16), layers=7):
    """The (H, W) of every upsampling stage: layers - 1 pairs, the last one img_hw itself."""
    H, W = int(img_hw[0]), int(img_hw[1])
    sx = (H / in_size[0]) ** (1.0 / (layers - 1))
    sy = (W / in_size[1]) ** (1.0 / (layers - 1))
    return [(int(np.ceil(sx ** n * in_size[0])), int(np.ceil(sy ** n * in_size[1]))) for n in range(1, layers - 1)] + [(H, W)]


class ConvDecoderParams:
    """The decoder's parameters as torch initialises them: `modules` is the nn.Sequential (CPU, module order: per stage
    Upsample, Conv2d, ReLU, BatchNorm2d; then Conv2d, ReLU, BatchNorm2d, Conv2d 1x1), `flat` one float32 bucket of all
    parameters in that order, `offsets[l]` = {"w", "b", "gamma", "beta"} -> (offset, shape) for the conv stages l = 0 ..
    layers - 1 and `head` = {"w", "b"}. `views(flat)` cuts any tensor of the bucket's layout (weights, gradients) up."""

    def __init__(self, img_shape, in_size=(16, 16), layers=7, channels=32):
        self.out_channels = int(img_shape[0])
        self.img_hw = (int(img_shape[1]), int(img_shape[2]))
        self.in_size, self.layers, self.channels = (int(in_size[0]), int(in_size[1])), int(layers), int(channels)
        if self.layers < 2:
            raise ValueError("ConvDecoder: at least two layers")
        self.sizes = decoder_sizes(self.img_hw, self.in_size, self.layers)
        ch, mods = self.channels, []
        for hw in self.sizes:
            mods += [nn.Upsample(size=hw, mode="nearest"), nn.Conv2d(ch, ch, 3, 1, padding=1, bias=True), nn.ReLU(),
                     nn.BatchNorm2d(ch, affine=True)]
        mods += [nn.Conv2d(ch, ch, 3, 1, padding=1, bias=True), nn.ReLU(), nn.BatchNorm2d(ch, affine=True),
                 nn.Conv2d(ch, self.out_channels, 1, 1, padding=0, bias=True)]
        self.modules = nn.Sequential(*mods)
        self.offsets, self.head, pos = [], None, 0
        convs = [m for m in self.modules if isinstance(m, nn.Conv2d)]
        norms = [m for m in self.modules if isinstance(m, nn.BatchNorm2d)]

        def take(t):
            nonlocal pos
            entry = (pos, tuple(t.shape))
            pos += t.numel()
            return entry

        for conv, bn in zip(convs[:-1], norms):
            self.offsets.append({"w": take(conv.weight), "b": take(conv.bias), "gamma": take(bn.weight),
                                 "beta": take(bn.bias)})
        self.head = {"w": take(convs[-1].weight), "b": take(convs[-1].bias)}
        self.numel = pos
        with torch.no_grad():
            self.flat = torch.cat([p.detach().reshape(-1) for p in self.modules.parameters()]).float().contiguous()
        assert self.flat.numel() == self.numel

    # stage l reads an image of in_hw(l) and writes one of out_hw(l); the last conv stage does not resample
    def out_hw(self, l):
        return self.sizes[min(l, len(self.sizes) - 1)]

    def in_hw(self, l):
        return self.in_size if l == 0 else self.out_hw(l - 1)

    def views(self, flat):
        def cut(entry):
            off, shape = entry
            return flat[off:off + int(np.prod(shape))].view(shape)
        return [{k: cut(v) for k, v in st.items()} for st in self.offsets], {k: cut(v) for k, v in self.head.items()}


class DecoderPlan:
    """Every device buffer of one decoder on `device`, allocated once: the stored activations a_l and statistics of each
    stage, the two gradient buffers the backward alternates between, the workspace of the reductions, x_hat."""

    def __init__(self, params, device):
        self.params = p = params
        if p.channels != 32:
            raise N.NativeLibraryError(f"the DIP kernels are built for 32 channels, not {p.channels}")
        self.device = torch.device(device)
        nst = p.layers
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)      # noqa: E731
        self.acts = [new(p.out_hw(l)[0] * p.out_hw(l)[1], 32) for l in range(nst)]
        self.stats = [new(128) for _ in range(nst)]
        biggest = max(max(h * w for h, w in p.sizes), p.in_size[0] * p.in_size[1])
        self.grads = [new(biggest, 32), new(biggest, 32)]
        words = 0
        for h, w in set(p.sizes):
            need = N.lib().sei_dip_work_floats(h, w, 32, p.out_channels)
            if need == 0:
                raise N.NativeLibraryError(f"sei_dip_work_floats refuses a {h} x {w} stage with {p.out_channels} outputs")
            words = max(words, need)
        self.work = new(words)
        self.x_hat = new(1, p.out_channels, *p.img_hw)
        self.z_cl = None


def _channels_last(z, plan):
    p = plan.params
    N.check_tensor(z.contiguous() if isinstance(z, torch.Tensor) else z, "z")
    if tuple(z.shape) != (1, p.channels) + tuple(p.in_size):
        raise ValueError(f"decoder: z of shape {tuple(z.shape)}, expected {(1, p.channels) + tuple(p.in_size)}")
    return z[0].permute(1, 2, 0).contiguous()


def _check_bucket(flat, plan, name):
    N.check_tensor(flat, name)
    if flat.numel() != plan.params.numel or flat.data_ptr() % 16:
        raise ValueError(f"{name}: expected the decoder's 16-byte aligned bucket of {plan.params.numel} floats")


def _forward_cl(plan, flat, z_cl):
    """The forward on a channels-last code; fills plan.acts / plan.stats / plan.x_hat."""
    p, base = plan.params, flat.data_ptr()
    at = lambda entry: base + 4 * entry[0]                   # noqa: E731
    src, ss = z_cl.data_ptr(), None
    for l, st in enumerate(p.offsets):
        (hi, wi), (ho, wo) = p.in_hw(l), p.out_hw(l)
        N.call("sei_dip_stage_fwd", src, ss, at(st["w"]), at(st["b"]), at(st["gamma"]), at(st["beta"]),
               plan.acts[l].data_ptr(), plan.stats[l].data_ptr(), hi, wi, ho, wo, 32, BN_EPS, plan.work.data_ptr())
        src, ss = plan.acts[l].data_ptr(), plan.stats[l].data_ptr() + 4 * 64
    H, W = p.img_hw
    N.call("sei_dip_head_fwd", src, ss, at(p.head["w"]), at(p.head["b"]), plan.x_hat.data_ptr(), H, W, 32, p.out_channels)
    return plan.x_hat


def _backward_cl(plan, flat, z_cl, g_x, grads):
    p, base, gbase = plan.params, flat.data_ptr(), grads.data_ptr()
    at = lambda entry: base + 4 * entry[0]                   # noqa: E731
    gat = lambda entry: gbase + 4 * entry[0]                 # noqa: E731
    last = p.layers - 1
    H, W = p.img_hw
    g, other = plan.grads
    N.call("sei_dip_head_bwd", g_x.data_ptr(), plan.acts[last].data_ptr(), plan.stats[last].data_ptr() + 4 * 64,
           at(p.head["w"]), g.data_ptr(), gat(p.head["w"]), gat(p.head["b"]), H, W, 32, p.out_channels,
           plan.work.data_ptr())
    for l in range(last, -1, -1):
        st = p.offsets[l]
        (hi, wi), (ho, wo) = p.in_hw(l), p.out_hw(l)
        N.call("sei_dip_stage_bwd_bn", g.data_ptr(), plan.acts[l].data_ptr(), plan.stats[l].data_ptr(), gat(st["gamma"]),
               gat(st["beta"]), ho, wo, 32, plan.work.data_ptr())
        prev = z_cl.data_ptr() if l == 0 else plan.acts[l - 1].data_ptr()
        ss = None if l == 0 else plan.stats[l - 1].data_ptr() + 4 * 64
        N.call("sei_dip_stage_bwd_weight", g.data_ptr(), prev, ss, gat(st["w"]), gat(st["b"]), hi, wi, ho, wo, 32,
               plan.work.data_ptr())
        if l > 0:                                            # nobody asks for the gradient of the code z
            N.call("sei_dip_stage_bwd_data", g.data_ptr(), at(st["w"]), other.data_ptr(), hi, wi, ho, wo, 32)
            g, other = other, g
    return grads


def decoder_forward(plan, flat, z):
    """G(z) for the float32 GPU bucket `flat` (ConvDecoderParams' layout) and the code z (1, 32, h0, w0), NCHW. Returns
    x_hat (1, C_out, H, W), a buffer of `plan` that the next call overwrites. No autograd."""
    _check_bucket(flat, plan, "flat")
    plan.z_cl = _channels_last(z, plan)
    return _forward_cl(plan, flat, plan.z_cl)


def decoder_backward(plan, flat, g_x, out=None):
    """The gradient of <g_x, G(z)> with respect to every parameter, in the bucket's layout (into `out` when given), for
    the forward that `decoder_forward(plan, flat, z)` just ran."""
    _check_bucket(flat, plan, "flat")
    if plan.z_cl is None:
        raise RuntimeError("decoder_backward: run decoder_forward on this plan first")
    N.check_tensor(g_x.contiguous() if isinstance(g_x, torch.Tensor) else g_x, "g_x")
    if g_x.shape != plan.x_hat.shape:
        raise ValueError(f"decoder_backward: g_x of shape {tuple(g_x.shape)}, x_hat is {tuple(plan.x_hat.shape)}")
    grads = torch.empty_like(flat) if out is None else out
    _check_bucket(grads, plan, "out")
    return _backward_cl(plan, flat, plan.z_cl, g_x.contiguous(), grads)


def _linear_operator(physics, x):
    """(op, transpose) of physics.A when it is one physics._ops operator, found on the autograd node of a probe call."""
    with torch.enable_grad():
        probe = physics.A(x.detach().clone().requires_grad_(True))
    node = probe.grad_fn
    if node is None or not hasattr(node, "op") or not hasattr(node, "transpose"):
        raise NotImplementedError("DeepImagePrior needs a physics whose A is one linear operator of physics._ops "
                                  "(its transpose is the gradient of the data-fit term)")
    return node.op, bool(node.transpose), tuple(probe.shape)


class DeepImagePrior(Module):
    """The reference's DeepImagePrior(physics, sr_factor, iterations) with deepinv's defaults (lr 5e-3, 32 channels, a
    16 x 16 code, 7 layers). `iterations_run` and `last_loss` (the data-fit value of the last step) describe the last
    forward. `trace=True` (measurements and tests) also keeps every step's value in `loss_history` and the fitted
    bucket in `final_weights`; otherwise nothing of the fit survives the forward."""

    def __init__(self, physics, sr_factor=None, iterations=4000, lr=5e-3, channels=32, in_size=None, graph=True,
                 trace=False):
        super().__init__()
        if physics is None:
            raise NotImplementedError("model kind 'DeepImagePrior' fits a decoder through the measurement operator: a "
                                      "folder of measurements has no operator to fit")
        self.physics = physics
        self.sr_factor = sr_factor
        self.iterations, self.lr, self.channels = int(iterations), float(lr), int(channels)
        self.in_size = [16, 16] if in_size is None else [int(in_size[0]), int(in_size[1])]
        self.layers = 7
        self.graph, self.trace = bool(graph), bool(trace)
        self.iterations_run, self.last_loss, self.loss_history, self.final_weights = 0, math.nan, [], None
        if self.iterations < 1:
            raise ValueError("DeepImagePrior: iterations >= 1")

    @torch.no_grad()
    def forward(self, y):
        N.check_tensor(y.contiguous() if isinstance(y, torch.Tensor) else y, "y")
        y = y.contiguous()
        if y.dim() != 4 or y.shape[0] != 1:
            raise ValueError(f"DeepImagePrior fits one measurement at a time: y of shape {tuple(y.shape)} is not (1, C, H, W)")
        C, H, W = y.shape[1:]
        if self.sr_factor is not None:                       # the reference scales whatever the task
            H, W = int(H * self.sr_factor), int(W * self.sr_factor)
        params = ConvDecoderParams((C, H, W), self.in_size, self.layers, self.channels)
        dev = y.device
        flat = params.flat.to(dev)
        z = torch.randn([self.channels] + self.in_size, device=dev)[None]
        plan = DecoderPlan(params, dev)
        z_cl = plan.z_cl = _channels_last(z, plan)
        op, transpose, y_shape = _linear_operator(self.physics, plan.x_hat.zero_())
        if y_shape != tuple(y.shape):
            raise ValueError(f"DeepImagePrior: A maps an image of shape {tuple(plan.x_hat.shape)} to {y_shape}, "
                             f"the measurement is {tuple(y.shape)}")
        n = y.numel()
        grads, m, v = torch.empty_like(flat), torch.zeros_like(flat), torch.zeros_like(flat)
        out2 = torch.zeros(2, dtype=torch.float32, device=dev)
        ga = torch.empty_like(y)
        red = torch.empty(N.SEI_REDUCE_BLOCKS, dtype=torch.float32, device=dev)
        hyper = torch.zeros(6, dtype=torch.float32, device=dev)
        history = torch.zeros(self.iterations, dtype=torch.float32, device=dev) if self.trace else None
        self.loss_history, self.final_weights = [], None
        in_hw = tuple(plan.x_hat.shape[-2:])

        def iteration():
            x_hat = _forward_cl(plan, flat, z_cl)
            y_hat = op.run(x_hat, transpose, None)
            N.call("sei_mse_loss", y_hat.data_ptr(), y.data_ptr(), n, 2.0 / n, 1.0 / n, out2.data_ptr(), ga.data_ptr(),
                   red.data_ptr())
            g_x = op.run(ga, not transpose, in_hw)
            _backward_cl(plan, flat, z_cl, g_x, grads)
            N.call("sei_dip_adam", flat.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr(), flat.numel(),
                   hyper.data_ptr())

        def scalars(step):
            N.call("sei_adam_scalars_to_device", self.lr, 0.9, 0.999, 1e-8, 0.0, step, hyper.data_ptr())

        self.iterations_run, captured = 0, None
        eager = self.iterations if not self.graph else min(WARMUP, self.iterations)
        for it in range(self.iterations):
            scalars(it + 1)
            if it < eager:
                iteration()
            else:
                if captured is None:                         # one linear chain on one stream
                    captured = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(captured):
                        iteration()
                captured.replay()
            if history is not None:
                history[it].copy_(out2[1])
            self.iterations_run = it + 1
        out = _forward_cl(plan, flat, z_cl).clone()
        self.last_loss = float(out2[1])                      # the one host read of the fit
        if self.trace:
            self.loss_history, self.final_weights = history.tolist(), flat.clone()
        del captured                                         # with the graph goes its memory pool
        return out
