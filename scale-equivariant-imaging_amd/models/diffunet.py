"""The diffusion U-Net denoiser of the DiffPIR_DiffUNet baseline (reference: src/models/diffpir.py, `model="DiffUNet"`):
deepinv 0.2.0's `DiffUNet(large_model=False)`, the guided-diffusion ("ADM") U-Net of the FFHQ-256 checkpoint. deepinv and
guided-diffusion are not part of the reference tree, so this restates them from recollection; parity with deepinv itself is
UNPINNED. The pinned truth is the float64 restatement in tests/diffunet_ref.py. Only the small model is here.

Network: ch = 128, multipliers (1, 1, 2, 2, 4, 4), one ResBlock per level, emb_dim = 512, learned variance (6 output channels,
of which only the noise estimate 0..2 is computed), attention with 64-wide heads in the legacy qkv order at 1/16 resolution
and in the middle. `plan()` lists the blocks with guided-diffusion's state-dict prefixes:

    input_blocks.0.0 conv3x3(3 -> 128); input_blocks.N.0 for N = 1 .. 11: RB(128), down-RB, RB(128), down-RB, RB(128 -> 256),
    down-RB, RB(256), down-RB, RB(256 -> 512) + Attn (input_blocks.9.1), down-RB, RB(512); every output is pushed as a skip.
    middle_block: RB(512), Attn, RB(512).
    output_blocks.N, each on cat(h, popped skip): RB(1024 -> 512); RB(1024 -> 512), up-RB; RB(1024 -> 512), Attn;
    RB(768 -> 512), Attn, up-RB; RB(768 -> 256); RB(512 -> 256), up-RB; RB(512 -> 256); RB(384 -> 256), up-RB; RB(384 -> 128);
    RB(256 -> 128), up-RB; RB(256 -> 128); RB(256 -> 128).
    out: GroupNorm, SiLU, conv3x3(128 -> 6).

    RB(x, e):  h = conv3x3(R(SiLU(GN32(x))));  (scale, shift) = chunk(Linear(SiLU(e)), 2);
               h = conv3x3(SiLU(GN32(h) (1 + scale) + shift));  result = skip(R(x)) + h
    with R the identity, the 2x2 average (down) or the 2x nearest repetition (up) and skip the identity or a biased 1x1
    convolution when the widths differ. GN32: 32 groups, eps 1e-5, affine.
    Attn(x):   qkv = conv1x1(GN32(x)); head h of C / 64 owns qkv channels [192 h, 192 h + 64) as q, then k, then v;
               a = softmax_s((q . k) / 8) v;  result = x + conv1x1(a).
    e = Linear(SiLU(Linear(cat(cos(t f), sin(t f))))), f_i = exp(-ln(10000) i / 64), i < 64.

Loading is strict and a mismatch prints both key lists. The user names the weights file (test.py --diffunet_weights: the
state dict of the FFHQ checkpoint that deepinv fetches); nothing is fetched here.

The denoiser call `forward(x, sigma)` for x in [0, 1] of shape (B, 3, H, W), H and W multiples of 32, sigma a positive float,
with the tables of models/diffpir.tables():

    alpha = 1 / (1 + 4 sigma^2);  z = sqrt(alpha) (2 x - 1);  s = 2 sigma sqrt(alpha);  t = first argmin_k |s1m[k] - s|
    eps = net(z, t)[:, :3];  x0 = clamp((z - s eps) / sa[t], -1, 1);  result = x0 / 2 + 0.5

(z is a variance-preserving diffusion state whose noise share is s). `eps(x, sigma)` returns the noise estimate itself.

Arithmetic follows models/_gemm.get_compute_dtype(self); the model's own default is "bf16":
- "bf16": the sei_adm_* family (csrc/adm_kernels.hip) on DRUNet's layout: a float32 trunk on the rows of a zero-bordered
  grid, bf16 grids with guard rows as the convolutions' inputs, bf16 weights converted once, float32 accumulation. Every
  matrix-product operand is rounded to bf16 -- convolution and 1x1 inputs and weights, q, k, v, the softmax probabilities --
  and nothing else is: the trunk, the skips, the GroupNorm statistics, SiLU, the modulation and the softmax are float32.
- "f32" (and "bf16x3", which maps to it): the parity mode, the same network from float32 entry points: the float32 outputs of
  sei_adm_gn_stats / sei_adm_gn_apply, nine row-shifted sei_gemm_f32_ex products per 3x3 convolution (one for a 1x1),
  sei_conv3x3_fwd for the head and the tail, torch expressions for attention's two products and the bias / residual
  additions. It makes no claim on speed.
The embedding MLPs (time_embed and every block's emb_layers, batched into one product) run once per call in torch.
"""
import math

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

import _native as N
from ._gemm import get_compute_dtype
from .diffpir import tables

CH, MULT, EMB, HEAD_DIM, ATTN_DS, GROUPS, EPS = 128, (1, 1, 2, 2, 4, 4), 512, 64, 16, 32, 1e-5
SAME, DOWN, UP = 0, 1, 2


def plan():
    """The blocks in execution order: ("rb", prefix, cin, cout, resample), ("attn", prefix, C), ("push",) after every
    input block and ("pop", width of the popped skip) ahead of every output block."""
    steps, widths, ch, ds = [("push",)], [CH], CH, 1
    n = 1
    for level, m in enumerate(MULT):
        steps.append(("rb", f"input_blocks.{n}.0", ch, m * CH, SAME))
        ch = m * CH
        if ds == ATTN_DS:
            steps.append(("attn", f"input_blocks.{n}.1", ch))
        steps.append(("push",))
        widths.append(ch)
        n += 1
        if level != len(MULT) - 1:
            steps += [("rb", f"input_blocks.{n}.0", ch, ch, DOWN), ("push",)]
            widths.append(ch)
            ds *= 2
            n += 1
    steps += [("rb", "middle_block.0", ch, ch, SAME), ("attn", "middle_block.1", ch), ("rb", "middle_block.2", ch, ch, SAME)]
    n = 0
    for level, m in list(enumerate(MULT))[::-1]:
        for i in range(2):
            skip = widths.pop()
            steps += [("pop", skip), ("rb", f"output_blocks.{n}.0", ch + skip, m * CH, SAME)]
            ch, sub = m * CH, 1
            if ds == ATTN_DS:
                steps.append(("attn", f"output_blocks.{n}.{sub}", ch))
                sub += 1
            if level and i == 1:
                steps.append(("rb", f"output_blocks.{n}.{sub}", ch, ch, UP))
                ds //= 2
            n += 1
    return steps


def expected_keys():
    """{state-dict key: shape} in guided-diffusion's naming."""
    keys = {"time_embed.0.weight": (EMB, CH), "time_embed.0.bias": (EMB,), "time_embed.2.weight": (EMB, EMB),
            "time_embed.2.bias": (EMB,), "input_blocks.0.0.weight": (CH, 3, 3, 3), "input_blocks.0.0.bias": (CH,)}
    for step in plan():
        if step[0] == "rb":
            _, p, cin, cout, _ = step
            keys.update({f"{p}.in_layers.0.weight": (cin,), f"{p}.in_layers.0.bias": (cin,),
                         f"{p}.in_layers.2.weight": (cout, cin, 3, 3), f"{p}.in_layers.2.bias": (cout,),
                         f"{p}.emb_layers.1.weight": (2 * cout, EMB), f"{p}.emb_layers.1.bias": (2 * cout,),
                         f"{p}.out_layers.0.weight": (cout,), f"{p}.out_layers.0.bias": (cout,),
                         f"{p}.out_layers.3.weight": (cout, cout, 3, 3), f"{p}.out_layers.3.bias": (cout,)})
            if cin != cout:
                keys.update({f"{p}.skip_connection.weight": (cout, cin, 1, 1), f"{p}.skip_connection.bias": (cout,)})
        elif step[0] == "attn":
            _, p, c = step
            keys.update({f"{p}.norm.weight": (c,), f"{p}.norm.bias": (c,), f"{p}.qkv.weight": (3 * c, c, 1),
                         f"{p}.qkv.bias": (3 * c,), f"{p}.proj_out.weight": (c, c, 1), f"{p}.proj_out.bias": (c,)})
    keys.update({"out.0.weight": (CH,), "out.0.bias": (CH,), "out.2.weight": (6, CH, 3, 3), "out.2.bias": (6,)})
    return keys


def timestep_embedding(t):
    """cat(cos(t f), sin(t f)) as a (1, 128) float32 tensor, evaluated in float64."""
    f = np.exp(-math.log(10000.0) * np.arange(64, dtype=np.float64) / 64)
    a = float(t) * f
    return torch.from_numpy(np.concatenate([np.cos(a), np.sin(a)])[None].astype(np.float32))


def timestep_of(sigma, tb=None):
    """(t, s, alpha) of the denoiser call at noise level sigma."""
    tb = tb or tables()
    alpha = 1.0 / (1.0 + 4.0 * sigma * sigma)
    s = 2.0 * sigma * math.sqrt(alpha)
    return int(np.abs(tb["s1m"].astype(np.float64) - s).argmin()), s, alpha


class CpuTensorError(N.NativeLibraryError, TypeError):
    """A CPU tensor where a GPU tensor is needed: the library's refusal, and a TypeError."""


class DiffUNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.compute_dtype = "bf16"
        for key, shape in expected_keys().items():            # one empty module per name on the path, the tensor at its end
            *path, leaf = key.split(".")
            mod = self
            for name in path:
                if name not in mod._modules:
                    mod.add_module(name, nn.Module())
                mod = mod._modules[name]
            mod.register_parameter(leaf, nn.Parameter(torch.zeros(shape), requires_grad=False))
        self.tables = tables()
        self._plan = plan()
        self._packed = {}
        self._work = {}

    # ---- weights ----
    @staticmethod
    def check_keys(state_dict):
        want, got = set(expected_keys()), set(state_dict)
        if want != got:
            raise KeyError(f"DiffUNet: the state dict does not fit. Missing keys: {sorted(want - got)}. "
                           f"Unexpected keys: {sorted(got - want)}")

    def load_state_dict(self, state_dict, strict=True):
        self.check_keys(state_dict)
        self._packed = {}
        return super().load_state_dict(state_dict, strict=True)

    def _apply(self, fn, *args, **kwargs):
        self._packed, self._work = {}, {}
        return super()._apply(fn, *args, **kwargs)

    @classmethod
    def from_file(cls, path, device):
        sd = torch.load(path, map_location="cpu", weights_only=True)
        cls.check_keys(sd)
        net = cls()
        net.load_state_dict(sd)
        return net.to(device).eval()

    def _weights(self, mode):
        """The weights as the kernels of `mode` read them, converted once."""
        if mode in self._packed:
            return self._packed[mode]
        out, emb_w, emb_b, at, off = {}, [], [], {}, 0
        for key, w in self.state_dict().items():
            w = w.detach().float()
            if ".emb_layers." in key:                         # batched into one product below
                (emb_w if key.endswith("weight") else emb_b).append(w)
                if key.endswith("weight"):
                    at[key[:-len(".emb_layers.1.weight")]] = (off, w.shape[0])
                    off += w.shape[0]
                continue
            if w.dim() == 3:                                  # attention's Conv1d (N, C, 1)
                w = w[..., None]
            if w.dim() != 4 or key.startswith("time_embed"):
                out[key] = w.contiguous()
            elif mode == "f32":
                if key == "input_blocks.0.0.weight":
                    out[key] = w.contiguous()                 # sei_conv3x3_fwd reads torch's layout
                elif key == "out.2.weight":
                    out[key] = w[:3].contiguous()
                else:
                    out[key] = w.permute(2, 3, 0, 1).reshape(-1, w.shape[0], w.shape[1]).contiguous()   # (taps, Cout, Cin)
            else:
                if key == "input_blocks.0.0.weight":          # 3 input channels, zero-padded to 32
                    w = F.pad(w, (0, 0, 0, 0, 0, 29))
                p = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)                     # tap-major (Cout, taps * Cin)
                if key == "out.2.weight":                     # the noise estimate's 3 rows, zero-padded to 16
                    p = F.pad(p[:3], (0, 0, 0, 13))
                out[key] = p.contiguous().to(torch.bfloat16)
        if mode == "f32":
            out["out.2.bias3"] = out["out.2.bias"][:3].contiguous()
        else:
            out["out.2.bias16"] = F.pad(out["out.2.bias"][:3], (0, 13)).contiguous()
        out["emb.weight"], out["emb.bias"], out["emb.at"] = torch.cat(emb_w).contiguous(), torch.cat(emb_b).contiguous(), at
        self._packed[mode] = out
        return out

    # ---- buffers: one per name and shape, kept; bf16 grids keep the zero border they were made with ----
    def _buf(self, name, rows, c, dtype, guard=0):
        """(row 0 of the buffer, the buffer): zeros once, `guard` rows in front and behind."""
        dev = next(self.parameters()).device
        key = (name, rows, c, dtype, guard, str(dev))
        if key not in self._work:
            buf = torch.zeros((rows + 2 * guard, c), dtype=dtype, device=dev)
            self._work[key] = (buf[guard:] if guard else buf, buf)
        return self._work[key]

    # ---- forward ----
    def _check(self, x):
        if isinstance(x, torch.Tensor) and not x.is_cuda:
            raise CpuTensorError(f"DiffUNet: x is on {x.device}: this build runs on MI355X only (HIP kernels, no CPU path)")
        N.check_tensor(x.contiguous() if isinstance(x, torch.Tensor) else x, "x")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"DiffUNet: expected (B, 3, H, W), got {tuple(x.shape)}")
        if x.shape[-2] % 32 or x.shape[-1] % 32:
            raise ValueError(f"DiffUNet: extents {tuple(x.shape[-2:])} are no multiples of 32")

    @torch.no_grad()
    def eps(self, x, sigma):
        """(eps, z, t, s): the noise estimate net(z, t)[:, :3] of the denoiser call and the state it was made for."""
        self._check(x)
        sigma = float(sigma)
        if not sigma > 0:
            raise ValueError(f"DiffUNet: sigma must be positive, got {sigma}")
        t, s, alpha = timestep_of(sigma, self.tables)
        z = (math.sqrt(alpha) * (2 * x.contiguous() - 1)).contiguous()
        return self.network(z, t), z, t, s

    @torch.no_grad()
    def forward(self, x, sigma):
        eps, z, t, s = self.eps(x, sigma)
        return ((z - s * eps) / float(self.tables["sa"][t])).clamp(-1, 1) / 2 + 0.5

    @torch.no_grad()
    def network(self, z, t):
        """net(z, t)[:, :3] for z (B, 3, H, W) float32 on the GPU and an integer timestep."""
        self._check(z)
        mode = get_compute_dtype(self)
        if mode not in ("bf16", "f32", "bf16x3"):
            raise ValueError(f"DiffUNet: unknown compute dtype {mode!r}")
        mode = "bf16" if mode == "bf16" else "f32"
        z = z.contiguous()
        if not N.aligned(z, to=4):
            z = z.clone()
        wts = self._weights(mode)
        e = timestep_embedding(t).to(z.device)
        e = F.linear(F.silu(F.linear(e, wts["time_embed.0.weight"], wts["time_embed.0.bias"])), wts["time_embed.2.weight"],
                     wts["time_embed.2.bias"])
        mods = F.linear(F.silu(e), wts["emb.weight"], wts["emb.bias"])
        run = _Run16(self, wts, mods, z) if mode == "bf16" else _Run32(self, wts, mods, z)
        return run.run()


class _Run:
    """One pass over `plan()`. A trunk is (float32 rows on the grid of (H, W), C, H, W)."""

    def __init__(self, net, wts, mods, z):
        self.net, self.w, self.z = net, wts, z
        self.B = B = z.shape[0]
        self.uid = 0
        # mods (1, sum of 2 cout): the same for every image (one timestep per call); kept per block as B contiguous rows
        flat = mods[0] if B == 1 else torch.cat([mods[0, o:o + n].repeat(B) for o, n in wts["emb.at"].values()])
        self.mods = net._buf("mods", flat.numel(), 1, torch.float32)[0].view(-1)
        self.mods.copy_(flat)

    def rows(self, h, w):
        return self.B * (h + 2) * (w + 2)

    def mod(self, prefix):
        """(B, 2 cout) scale | shift of the block: its piece of the kept buffer that __init__ laid out block by block."""
        off, n = self.w["emb.at"][prefix]
        return self.mods[self.B * off:self.B * (off + n)]

    def stats(self, xa, ca, xb, cb, h, w):
        st = self.net._buf("stats", self.B, 2 * GROUPS, torch.float32)[0]       # consumed by the launch behind it
        part = self.net._buf("stats.part", self.B, N.lib().sei_adm_gn_part_floats(h, w), torch.float32)[0]
        N.call("sei_adm_gn_stats", xa.data_ptr(), ca, N.ptr(xb), cb, self.B, h, w, EPS, st.data_ptr(), part.data_ptr())
        return st

    def apply(self, xa, ca, xb, cb, st, norm, mod, silu, h, w, resample, y16, y32):
        g = self.w[norm + ".weight"] if norm else None
        b = self.w[norm + ".bias"] if norm else None
        N.call("sei_adm_gn_apply", xa.data_ptr(), ca, N.ptr(xb), cb, N.ptr(st), N.ptr(g), N.ptr(b), N.ptr(mod), silu, self.B,
               h, w, resample, N.ptr(y16), N.ptr(y32))

    def fresh(self, rows, c):
        """A trunk buffer of this pass's own (skips outlive the block that made them)."""
        self.uid += 1
        return self.net._buf(f"trunk{self.uid}", rows, c, torch.float32)[0]

    def run(self):
        h, w = self.z.shape[-2:]
        x, c = self.head(h, w), CH
        skips, popped = [], None
        for step in self.net._plan:
            if step[0] == "push":
                skips.append((x, c))
            elif step[0] == "pop":
                popped = skips.pop()
            elif step[0] == "rb":
                _, prefix, cin, cout, how = step
                xb, cb = popped if popped is not None else (None, 0)
                popped = None
                assert c + cb == cin
                x = self.rb(prefix, x, c, xb, cb, cout, how, h, w)
                c = cout
                if how == DOWN:
                    h, w = h // 2, w // 2
                elif how == UP:
                    h, w = 2 * h, 2 * w
            else:
                x = self.attn(step[1], x, c, h, w)
        return self.tail(x, h, w)


def _out_extents(h, w, how):
    return (h // 2, w // 2) if how == DOWN else (2 * h, 2 * w) if how == UP else (h, w)


class _Run16(_Run):
    """"bf16": the sei_adm_* kernels."""

    def grid(self, name, h, w, c):
        return self.net._buf(f"{name}.{self.B}x{h}x{w}", self.rows(h, w), c, torch.bfloat16, guard=w + 3)[0]

    def conv(self, x16, key, cin, cout, taps, h, w, res=None, out32=None, out16=None):
        N.call("sei_adm_conv", x16.data_ptr(), self.w[key + ".weight"].data_ptr(), self.w[key + ".bias"].data_ptr(), cin, cout,
               taps, self.B, h, w, N.ptr(res), N.ptr(out32), N.ptr(out16))

    def head(self, h, w):
        g = self.grid("image", h, w, 32)
        N.call("sei_adm_pack_image", self.z.data_ptr(), g.data_ptr(), self.B, h, w)
        x = self.fresh(self.rows(h, w), CH)
        self.conv(g, "input_blocks.0.0", 32, CH, 9, h, w, out32=x)
        return x

    def rb(self, prefix, xa, ca, xb, cb, cout, how, h, w):
        cin = ca + cb
        ho, wo = _out_extents(h, w, how)
        rows = self.rows(ho, wo)
        y = self.grid("a", ho, wo, cin)
        self.apply(xa, ca, xb, cb, self.stats(xa, ca, xb, cb, h, w), prefix + ".in_layers.0", None, 1, h, w, how, y, None)
        hid = self.net._buf("hidden", rows, cout, torch.float32)[0]
        self.conv(y, prefix + ".in_layers.2", cin, cout, 9, ho, wo, out32=hid)
        y2 = self.grid("b", ho, wo, cout)
        self.apply(hid, cout, None, 0, self.stats(hid, cout, None, 0, ho, wo), prefix + ".out_layers.0", self.mod(prefix), 1,
                   ho, wo, SAME, y2, None)
        if cin != cout:                                       # the 1x1 skip reads a bf16 copy of the (concatenated) input
            raw = self.grid("c", ho, wo, cin)
            self.apply(xa, ca, xb, cb, None, None, None, 0, h, w, how, raw, None)
            res = self.net._buf("skip", rows, cout, torch.float32)[0]
            self.conv(raw, prefix + ".skip_connection", cin, cout, 1, ho, wo, out32=res)
        elif how != SAME:
            res = self.net._buf("skip", rows, cout, torch.float32)[0]
            self.apply(xa, ca, None, 0, None, None, None, 0, h, w, how, None, res)
        else:
            res = xa
        out = self.fresh(rows, cout)
        self.conv(y2, prefix + ".out_layers.3", cout, cout, 9, ho, wo, res=res, out32=out)
        return out

    def attn(self, prefix, x, c, h, w):
        rows = self.rows(h, w)
        y = self.grid("a", h, w, c)
        self.apply(x, c, None, 0, self.stats(x, c, None, 0, h, w), prefix + ".norm", None, 0, h, w, SAME, y, None)
        qkv = self.net._buf("qkv", rows, 3 * c, torch.bfloat16)[0]
        self.conv(y, prefix + ".qkv", c, 3 * c, 1, h, w, out16=qkv)
        a = self.net._buf("attn", rows, c, torch.bfloat16)[0]
        N.call("sei_adm_attention", qkv.data_ptr(), c, self.B, h, w, a.data_ptr())
        out = self.fresh(rows, c)
        self.conv(a, prefix + ".proj_out", c, c, 1, h, w, res=x, out32=out)
        return out

    def tail(self, x, h, w):
        y = self.grid("a", h, w, CH)
        self.apply(x, CH, None, 0, self.stats(x, CH, None, 0, h, w), "out.0", None, 1, h, w, SAME, y, None)
        out = torch.empty_like(self.z)
        N.call("sei_adm_tail", y.data_ptr(), self.w["out.2.weight"].data_ptr(), self.w["out.2.bias16"].data_ptr(), CH, self.B, h,
               w, out.data_ptr())
        return out


class _Run32(_Run):
    """"f32": the parity mode. Convolution inputs are float32 grids with w + 3 guard rows, as the bf16 mode's."""

    def grid(self, name, h, w, c):
        return self.net._buf(f"{name}.{self.B}x{h}x{w}", self.rows(h, w), c, torch.float32, guard=w + 3)

    def conv(self, grid, key, h, w, res=None, out=None):
        """conv + bias [+ res] on the grid's rows from the per-tap matrices (taps, Cout, Cin); border rows hold sums that
        nothing reads."""
        x0, buf = grid
        wt, rows, wp, guard = self.w[key + ".weight"], self.rows(h, w), w + 2, w + 3
        cout, cin = wt.shape[1], wt.shape[2]
        out = torch.empty((rows, cout), dtype=torch.float32, device=buf.device) if out is None else out
        taps = [(1, 1)] if wt.shape[0] == 1 else [(ky, kx) for ky in range(3) for kx in range(3)]
        for i, (ky, kx) in enumerate(taps):
            off = guard + (ky - 1) * wp + (kx - 1)
            N.call("sei_gemm_f32_ex", buf[off:off + rows].data_ptr(), wt[i].data_ptr(), out.data_ptr(), rows, cout, cin, 0, 1,
                   5 if i else 0, None, None, None, None, 1, 0, 0, 0, 0)
        out += self.w[key + ".bias"]
        if res is not None:
            out += res
        return out

    def interior(self, x, c, h, w):
        return x.view(self.B, h + 2, w + 2, c)[:, 1:-1, 1:-1]

    def head(self, h, w):
        y = torch.empty((self.B, h, w, CH), dtype=torch.float32, device=self.z.device)
        N.call("sei_conv3x3_fwd", self.z.data_ptr(), self.w["input_blocks.0.0.weight"].data_ptr(),
               self.w["input_blocks.0.0.bias"].data_ptr(), None, y.data_ptr(), self.B, h, w, 3, CH, 1, 0, 0)
        x = self.fresh(self.rows(h, w), CH)
        self.interior(x, CH, h, w).copy_(y)
        return x

    def rb(self, prefix, xa, ca, xb, cb, cout, how, h, w):
        cin = ca + cb
        ho, wo = _out_extents(h, w, how)
        rows = self.rows(ho, wo)
        y = self.grid("a", ho, wo, cin)
        self.apply(xa, ca, xb, cb, self.stats(xa, ca, xb, cb, h, w), prefix + ".in_layers.0", None, 1, h, w, how, None, y[0])
        hid = self.conv(y, prefix + ".in_layers.2", ho, wo)
        y2 = self.grid("b", ho, wo, cout)
        self.apply(hid, cout, None, 0, self.stats(hid, cout, None, 0, ho, wo), prefix + ".out_layers.0", self.mod(prefix), 1,
                   ho, wo, SAME, None, y2[0])
        if cin != cout:
            raw = self.grid("c", ho, wo, cin)
            self.apply(xa, ca, xb, cb, None, None, None, 0, h, w, how, None, raw[0])
            res = self.conv(raw, prefix + ".skip_connection", ho, wo)
        elif how != SAME:
            res = torch.empty((rows, cout), dtype=torch.float32, device=xa.device)
            self.apply(xa, ca, None, 0, None, None, None, 0, h, w, how, None, res)
        else:
            res = xa
        return self.conv(y2, prefix + ".out_layers.3", ho, wo, res=res, out=self.fresh(rows, cout))

    def attn(self, prefix, x, c, h, w):
        B, T, heads = self.B, h * w, c // HEAD_DIM
        y = self.grid("a", h, w, c)
        self.apply(x, c, None, 0, self.stats(x, c, None, 0, h, w), prefix + ".norm", None, 0, h, w, SAME, None, y[0])
        qkv = self.interior(self.conv(y, prefix + ".qkv", h, w), 3 * c, h, w).reshape(B, T, heads, 3, HEAD_DIM)
        q, k, v = (qkv[:, :, :, i].permute(0, 2, 1, 3) for i in range(3))                 # (B, heads, T, 64)
        a = self.grid("d", h, w, c)
        dst = self.interior(a[0][:self.rows(h, w)], c, h, w)
        for i in range(B):                                    # one image at a time: the products' shapes, and with them the
            p = torch.softmax(torch.matmul(q[i], k[i].transpose(-1, -2)) * (1.0 / math.sqrt(HEAD_DIM)), dim=-1)   # bits, do
            dst[i].copy_(torch.matmul(p, v[i]).permute(1, 0, 2).reshape(h, w, c))                                 # not depend on B
        return self.conv(a, prefix + ".proj_out", h, w, res=x, out=self.fresh(self.rows(h, w), c))

    def tail(self, x, h, w):
        y = self.net._buf("tail", self.rows(h, w), CH, torch.float32)[0]
        self.apply(x, CH, None, 0, self.stats(x, CH, None, 0, h, w), "out.0", None, 1, h, w, SAME, None, y)
        t = self.interior(y, CH, h, w).contiguous()
        out = torch.empty_like(self.z)
        N.call("sei_conv3x3_fwd", t.data_ptr(), self.w["out.2.weight"].data_ptr(), self.w["out.2.bias3"].data_ptr(), None,
               out.data_ptr(), self.B, h, w, CH, 3, 0, 1, 0)
        return out
