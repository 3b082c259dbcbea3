"""The DRUNet denoiser (Zhang et al., "Plug-and-Play Image Restoration with Deep Denoiser Prior"; KAIR's
`network_unet.UNetRes`, which deepinv 0.2 wraps as `deepinv.models.DRUNet`) that the PlugAndPlay baseline calls
(reference: src/models/pnp.py). deepinv is not part of the reference tree, so this restates its documented behaviour;
parity with deepinv itself is UNPINNED. The pinned truth is the float64 restatement in tests/drunet_ref.py.

Network, for in_channels = out_channels = 3, nc = (64, 128, 256, 512), nb = 4, no bias anywhere, ReLU:

    x0 = cat(x, sigma * ones(B, 1, H, W))                       sigma a Python float
    x1 = m_head(x0)                                             conv3x3 4 -> nc0
    x2 = m_down1(x1); x3 = m_down2(x2); x4 = m_down3(x3)        nb ResBlocks, then a 2x2 stride-2 convolution
    x  = m_body(x4)                                             nb ResBlocks at nc3
    x  = m_up3(x + x4); x = m_up2(x + x3); x = m_up1(x + x2)    a 2x2 stride-2 transposed convolution, then nb ResBlocks
    out = m_tail(x + x1)                                        conv3x3 nc0 -> 3

with ResBlock(x) = x + conv(relu(conv(x))) and zero padding 1 on every 3x3 convolution. The state-dict keys are KAIR's
(`m_head.weight`, `m_down1.0.res.0.weight`, .., `m_down1.4.weight`, `m_body.0.res.2.weight`, `m_up3.0.weight` in
ConvTranspose2d's (Cin, Cout, 2, 2) layout, .., `m_tail.weight`): 64 tensors and 32,640,960 parameters with the defaults.
Nobody here could check the names against the published file, so loading is strict and a mismatch prints both key lists.
The user names the weights file (test.py --drunet_weights); nothing is fetched.

Image extents, as deepinv's eval-mode forward: both axes multiples of 8 and above 31 run directly; with an axis below 32
the image is replicate-padded at the bottom and right to multiples of 16, run and cropped; anything else is "onesplit"
with refield 64: the four corner pieces of extent p(n) = (n // 2 // 64 + 1) * 64 per axis, each output quadrant (cut at
h // 2, w // 2) from its own piece. A piece that does not fit the image raises ValueError (deepinv dies on a shape error).

Arithmetic follows models/_gemm.get_compute_dtype(self); the model's own default is "bf16":
- "bf16": the sei_drunet_* family (csrc/drunet_kernels.hip): bf16 activations on zero-bordered channels-last grids, a
  float32 residual trunk, bf16 weights converted once, float32 accumulation. Every convolution input and every weight is
  rounded to bf16; nothing else is.
- "f32" (and "bf16x3", which maps to it): the parity mode, the same network from existing float32 entry points --
  sei_conv3x3_fwd for the head and the tail, nine row-shifted sei_gemm_f32 products on sei_pad_nhwc's grid for the wide
  3x3 convolutions (sei_conv3x3_fwd holds its weights in LDS and stops below 64 x 64 channels), one sei_gemm_f32 for
  each 2x2 convolution with torch views for the pixel shuffles. It makes no claim on speed.

The vector-Jacobian product (the DPS baseline, models/dps.py, differentiates its data term through the denoiser):
`forward_taped(x, sigma) -> (out, tape)` is `forward` (the same launches, the same bits) with every ResBlock's ReLU output
kept in a buffer of its own instead of the shared one, and `vjp(tape, g) -> gx` is J(x)^T g for g of x's shape, without
torch autograd. The transposed network is the network again: tail^T takes the head's place, the up stages (blocks in
reverse, then the transposed 2x2 layer) the down stages', the body its own, the down stages the up stages', head^T the
tail's (the constant sigma channel needs no gradient), and the U-Net skips fan the gradient out where they fanned the
activations in: the gradient at the input of each m_up* transposed convolution is also the gradient of the skip tensor
of that level, kept in the level's float32 skip buffer and added where the backward reaches that tensor from the down path
(m_tail(x + x1) and m_body(x4) + x4 likewise). A ResBlock's backward is G_in = G_out + conv1^T([mid > 0] conv2^T(G_out)).
- "bf16": the gradient flows as the activations do -- a float32 trunk, a bf16 copy as every convolution's input, bf16
  transposed weights packed once, float32 accumulation, no split-K and no atomics: the same bits on every run and at every
  batch position. The operators are the forward's kernels with repacked weights (conv3x3^T: taps flipped, Cin / Cout
  swapped; down^T on sei_drunet_up; up^T on sei_drunet_down; tail^T on sei_drunet_head with sigma = 0; head^T on
  sei_drunet_tail) and one new launch, sei_drunet_conv3x3_masked, Y16 = bf16(conv(G) [mid > 0]) from the taped bf16 grid.
- "f32" / "bf16x3": the same product from _conv32 with transposed per-tap matrices, sei_gemm_f32_ex with the roles swapped
  for the 2x2 layers, sei_conv3x3_fwd's transposed switch for the ends and torch for the masks. No claim on speed.
The tape of the bf16 mode is one bf16 grid per ResBlock: 2 (H + 2)(W + 2) nb (2 nc0 + nc1 / 2 + nc2 / 8 + nc3 / 64) bytes per
image, 187 MB for 256 x 384 with the defaults. Tape buffers are kept per extents and reused: a tape is valid until the next
forward_taped of the same batch and extents. Runnable extents run directly; onesplit extents run as the adjoint of the
forward's gather (g's quadrants scattered into the four pieces, one product over the 4B batch, the pieces summed back
into the image; `tape.masks()` is then of that 4B batch). The replicate-pad path (an axis below 32) raises ValueError in
forward_taped: no workload has it.
"""
import torch
from torch import nn
from torch.nn import functional as F

import _native as N
from ._gemm import get_compute_dtype

REFIELD = 64
_WIDTHS = (64, 128, 256, 512)
_TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]


class ResBlock(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.res = nn.Sequential(nn.Conv2d(c, c, 3, 1, 1, bias=False), nn.ReLU(), nn.Conv2d(c, c, 3, 1, 1, bias=False))


def expected_keys(nc=(64, 128, 256, 512), nb=4):
    """{state-dict key: shape} of DRUNet(nc, nb), in KAIR's naming."""
    keys = {"m_head.weight": (nc[0], 4, 3, 3)}
    for lvl in range(3):
        for i in range(nb):
            for j in (0, 2):
                keys[f"m_down{lvl + 1}.{i}.res.{j}.weight"] = (nc[lvl], nc[lvl], 3, 3)
        keys[f"m_down{lvl + 1}.{nb}.weight"] = (nc[lvl + 1], nc[lvl], 2, 2)
    for i in range(nb):
        for j in (0, 2):
            keys[f"m_body.{i}.res.{j}.weight"] = (nc[3], nc[3], 3, 3)
    for lvl in (3, 2, 1):
        keys[f"m_up{lvl}.0.weight"] = (nc[lvl], nc[lvl - 1], 2, 2)
        for i in range(1, nb + 1):
            for j in (0, 2):
                keys[f"m_up{lvl}.{i}.res.{j}.weight"] = (nc[lvl - 1], nc[lvl - 1], 3, 3)
    keys["m_tail.weight"] = (3, nc[0], 3, 3)
    return keys


def piece_extent(n):
    return (n // 2 // REFIELD + 1) * REFIELD


def onesplit_plan(h, w):
    """The four corner pieces of an h x w image: [(piece rows, piece columns, output rows, output columns, rows inside the
    piece, columns inside the piece)], all slices. Raises ValueError when a piece does not fit the image."""
    ph, pw = piece_extent(h), piece_extent(w)
    if ph > h or pw > w:
        raise ValueError(f"DRUNet: a {h} x {w} image splits into {ph} x {pw} pieces, which do not fit it")
    rows = [(slice(0, ph), slice(0, h // 2), slice(0, h // 2)), (slice(h - ph, h), slice(h // 2, h), slice(ph - h + h // 2, ph))]
    cols = [(slice(0, pw), slice(0, w // 2), slice(0, w // 2)), (slice(w - pw, w), slice(w // 2, w), slice(pw - w + w // 2, pw))]
    return [(r[0], c[0], r[1], c[1], r[2], c[2]) for r in rows for c in cols]


def runnable(h, w):
    return h % 8 == 0 and w % 8 == 0 and h > 31 and w > 31


class Tape:
    """What `DRUNet.vjp` needs of one `forward_taped`: per ResBlock, in network order (m_down1 .. m_down3, m_body, m_up3 ..
    m_up1), the ReLU output of its first convolution -- bf16 zero-bordered grids in "bf16" mode, float32 NHWC in "f32"."""

    def __init__(self, mode, shape, plan, batch):
        self.mode, self.shape, self.plan, self.batch = mode, tuple(shape), plan, batch      # shape: of the batch that ran
        self.mids, self.grids = [], None                      # grids: the bf16 mode's buffers, handed out block by block

    def masks(self):
        """[mid > 0] of every ResBlock as bool NCHW tensors, in network order."""
        if self.mode != "bf16":
            return [(m > 0).permute(0, 3, 1, 2) for m in self.mids]
        B, out = self.shape[0], []
        for grid, h, w in self.mids:
            rows = B * (h + 2) * (w + 2)
            out.append((grid[:rows].view(B, h + 2, w + 2, -1)[:, 1:-1, 1:-1] > 0).permute(0, 3, 1, 2))
        return out


class DRUNet(nn.Module):
    def __init__(self, nc=(64, 128, 256, 512), nb=4):
        super().__init__()
        nc = tuple(int(c) for c in nc)
        if len(nc) != 4 or any(c not in _WIDTHS for c in nc) or nb < 1:
            raise ValueError(f"DRUNet: four widths out of {_WIDTHS} and nb >= 1, got {nc} and {nb}")
        self.nc, self.nb = nc, int(nb)
        self.compute_dtype = "bf16"
        self.m_head = nn.Conv2d(4, nc[0], 3, 1, 1, bias=False)
        for lvl in range(3):
            setattr(self, f"m_down{lvl + 1}", nn.Sequential(*[ResBlock(nc[lvl]) for _ in range(nb)],
                                                            nn.Conv2d(nc[lvl], nc[lvl + 1], 2, 2, 0, bias=False)))
        self.m_body = nn.Sequential(*[ResBlock(nc[3]) for _ in range(nb)])
        for lvl in (3, 2, 1):
            setattr(self, f"m_up{lvl}", nn.Sequential(nn.ConvTranspose2d(nc[lvl], nc[lvl - 1], 2, 2, 0, bias=False),
                                                      *[ResBlock(nc[lvl - 1]) for _ in range(nb)]))
        self.m_tail = nn.Conv2d(nc[0], 3, 3, 1, 1, bias=False)
        self.requires_grad_(False)
        self._packed = {}            # mode -> {key: packed weight}
        self._buffers_by_shape = {}
        self._tapes_by_shape = {}

    # ---- weights ----
    @staticmethod
    def check_keys(state_dict, nc, nb):
        want, got = set(expected_keys(nc, nb)), set(state_dict)
        if want != got:
            raise KeyError(f"DRUNet{tuple(nc), nb}: the state dict does not fit. Missing keys: {sorted(want - got)}. "
                           f"Unexpected keys: {sorted(got - want)}")

    def load_state_dict(self, state_dict, strict=True):
        self.check_keys(state_dict, self.nc, self.nb)
        self._packed = {}
        return super().load_state_dict(state_dict, strict=True)

    def _apply(self, fn, *args, **kwargs):
        self._packed, self._buffers_by_shape, self._tapes_by_shape = {}, {}, {}
        return super()._apply(fn, *args, **kwargs)

    @classmethod
    def from_file(cls, path, device, nc=(64, 128, 256, 512), nb=4):
        sd = torch.load(path, map_location="cpu", weights_only=True)
        cls.check_keys(sd, nc, nb)
        net = cls(nc, nb)
        net.load_state_dict(sd)
        return net.to(device).eval()

    def _weights(self, mode):
        """The weights as the kernels of `mode` read them, converted once."""
        if mode in self._packed:
            return self._packed[mode]
        sd, out = self.state_dict(), {}
        for key, w in sd.items():
            w = w.detach().float()
            if key.startswith("m_up") and w.shape[-1] == 2:                  # (Cin, Cout, 2, 2) -> (4 Cout, Cin)
                p = w.permute(2, 3, 1, 0).reshape(4 * w.shape[1], w.shape[0])
            elif mode == "f32" and key in ("m_head.weight", "m_tail.weight"):
                p = w                                                        # sei_conv3x3_fwd reads torch's layout
            elif mode == "f32" and w.shape[-1] == 3:
                p = w.permute(2, 3, 0, 1).reshape(9, w.shape[0], w.shape[1])  # one (Cout, Cin) matrix per tap
            else:
                if key == "m_head.weight":                                   # 4 input channels, zero-padded to 32
                    w = F.pad(w, (0, 0, 0, 0, 0, 28))
                p = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)             # tap-major (Cout, taps * Cin)
                if key == "m_tail.weight":                                   # 3 output channels, zero-padded to 16
                    p = F.pad(p, (0, 0, 0, 13))
            out[key] = p.contiguous().to(torch.bfloat16 if mode == "bf16" else torch.float32)
        self._packed[mode] = out
        return out

    @staticmethod
    def pack_transposed(key, w, mode):
        """The weight `key` (float32, torch's layout) as the kernel that runs its layer's TRANSPOSE in `mode` reads it."""
        if key.startswith("m_up") and w.shape[-1] == 2:       # (Cin, Cout, 2, 2): its transpose is the Conv2d of that weight
            return w.permute(0, 2, 3, 1).reshape(w.shape[0], 4 * w.shape[1])     # tap-major (Cin, 4 Cout): a down layer
        if w.shape[-1] == 2:                                  # (Cout, Cin, 2, 2): its transpose is the ConvTranspose2d
            return w.permute(2, 3, 1, 0).reshape(4 * w.shape[1], w.shape[0])     # (4 Cin, Cout): an up layer
        if mode == "f32" and key == "m_tail.weight":
            return w                                          # sei_conv3x3_fwd's transposed switch reads the forward weight
        if mode == "f32" and key == "m_head.weight":
            return w[:, :3]                                   # (the constant sigma channel needs no gradient)
        wt = (w[:, :3] if key == "m_head.weight" else w).flip(2, 3).transpose(0, 1)       # conv3x3^T as a conv3x3
        if mode == "f32":
            return wt.permute(2, 3, 0, 1).reshape(9, wt.shape[0], wt.shape[1])
        if key == "m_tail.weight":                            # 3 input channels, zero-padded to the head kernel's 32
            wt = F.pad(wt, (0, 0, 0, 0, 0, 29))
        p = wt.permute(0, 2, 3, 1).reshape(wt.shape[0], -1)
        return F.pad(p, (0, 0, 0, 13)) if key == "m_head.weight" else p          # 3 output channels, zero-padded to 16

    def _weights_t(self, mode):
        """The transposed weights as the kernels of `mode` read them, converted once."""
        if mode + "^T" not in self._packed:
            dtype = torch.bfloat16 if mode == "bf16" else torch.float32
            self._packed[mode + "^T"] = {key: self.pack_transposed(key, w.detach().float(), mode).contiguous().to(dtype)
                                         for key, w in self.state_dict().items()}
        return self._packed[mode + "^T"]

    # ---- forward ----
    @torch.no_grad()
    def forward_taped(self, x, sigma):
        """(forward(x, sigma), the tape `vjp` needs)."""
        N.check_tensor(x.contiguous() if isinstance(x, torch.Tensor) else x, "x")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"DRUNet: expected (B, 3, H, W), got {tuple(x.shape)}")
        x, sigma = x.contiguous(), float(sigma)
        B, _, h, w = x.shape
        if h < 32 or w < 32:
            raise ValueError(f"DRUNet.forward_taped: {h} x {w} would run replicate-padded, which has no backward here")
        mode = "bf16" if get_compute_dtype(self) == "bf16" else "f32"
        if runnable(h, w):
            tape = Tape(mode, x.shape, None, B)
            return self._run(x, sigma, tape), tape
        plan = onesplit_plan(h, w)
        xs = torch.cat([x[..., pr, pc] for pr, pc, *_ in plan], 0).contiguous()
        tape = Tape(mode, xs.shape, (plan, h, w), B)
        pieces = self._run(xs, sigma, tape)
        out = torch.empty_like(x)
        for q, (_, _, orow, ocol, irow, icol) in enumerate(plan):
            out[..., orow, ocol] = pieces[q * B:(q + 1) * B][..., irow, icol]
        return out, tape

    @torch.no_grad()
    def vjp(self, tape, g):
        """J(x)^T g for the x of `tape`'s forward_taped: g and the result have x's shape."""
        N.check_tensor(g.contiguous() if isinstance(g, torch.Tensor) else g, "g")
        g = g.contiguous()
        run = self._vjp_bf16 if tape.mode == "bf16" else self._vjp_f32
        if tape.plan is None:
            if tuple(g.shape) != tape.shape:
                raise ValueError(f"DRUNet.vjp: g is {tuple(g.shape)}, the tape's input was {tape.shape}")
            return run(tape, g if N.aligned(g, to=4) else g.clone())
        (plan, h, w), B = tape.plan, tape.batch
        if tuple(g.shape) != (B, 3, h, w):
            raise ValueError(f"DRUNet.vjp: g is {tuple(g.shape)}, the tape's input was {(B, 3, h, w)}")
        gs = torch.zeros(tape.shape, dtype=torch.float32, device=g.device)       # the adjoint of the forward's gather
        for q, (_, _, orow, ocol, irow, icol) in enumerate(plan):
            gs[q * B:(q + 1) * B][..., irow, icol] = g[..., orow, ocol]
        gp = run(tape, gs)
        gx = torch.zeros_like(g)
        for q, (pr, pc, *_) in enumerate(plan):
            gx[..., pr, pc] += gp[q * B:(q + 1) * B]
        return gx

    @torch.no_grad()
    def forward(self, x, sigma):
        N.check_tensor(x.contiguous() if isinstance(x, torch.Tensor) else x, "x")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"DRUNet: expected (B, 3, H, W), got {tuple(x.shape)}")
        x, sigma = x.contiguous(), float(sigma)
        h, w = x.shape[-2:]
        if runnable(h, w):
            return self._run(x, sigma)
        if h < 32 or w < 32:
            hp, wp = -(-h // 16) * 16, -(-w // 16) * 16
            return self._run(F.pad(x, (0, wp - w, 0, hp - h), mode="replicate").contiguous(), sigma)[..., :h, :w].contiguous()
        plan = onesplit_plan(h, w)
        B = x.shape[0]
        pieces = self._run(torch.cat([x[..., pr, pc] for pr, pc, *_ in plan], 0).contiguous(), sigma)
        out = torch.empty_like(x)
        for q, (_, _, orow, ocol, irow, icol) in enumerate(plan):
            out[..., orow, ocol] = pieces[q * B:(q + 1) * B][..., irow, icol]
        return out

    def _run(self, x, sigma, tape=None):
        mode = get_compute_dtype(self)
        if mode not in ("bf16", "f32", "bf16x3"):
            raise ValueError(f"DRUNet: unknown compute dtype {mode!r}")
        if x.shape[-2] % 8 or x.shape[-1] % 8:
            raise ValueError(f"DRUNet: extents {tuple(x.shape[-2:])} are no multiples of 8")
        if not N.aligned(x, to=4):
            x = x.clone()
        return self._run_bf16(x, sigma, tape) if mode == "bf16" else self._run_f32(x, sigma, tape)

    # "bf16": the fused family
    def _grids(self, B, H, W, device):
        key = (B, H, W, str(device))
        if key not in self._buffers_by_shape:
            lv = []
            for lvl, c in enumerate(self.nc):
                h, w = H >> lvl, W >> lvl
                rows, guard = B * (h + 2) * (w + 2), w + 3
                ya, yb = (torch.zeros((rows + 2 * guard, c), dtype=torch.bfloat16, device=device) for _ in range(2))
                t, skip = (torch.zeros((rows, c), dtype=torch.float32, device=device) for _ in range(2))
                lv.append((ya[guard:], yb[guard:], t, skip, ya, yb))
            nbytes = N.lib().sei_drunet_work_bytes(B, H, W)
            if nbytes == 0:
                raise N.NativeLibraryError(f"sei_drunet_head refuses {B} images of {H} x {W}")
            self._buffers_by_shape[key] = (lv, torch.zeros(nbytes, dtype=torch.uint8, device=device))
        return self._buffers_by_shape[key]

    def _tape_grids(self, B, H, W, device):
        """One bf16 grid (with its guard rows) per ResBlock, in network order: [(row 0 of the grid, h, w, the buffer)]."""
        key = (B, H, W, str(device))
        if key not in self._tapes_by_shape:
            grids = []
            for lvl in (0, 1, 2, 3, 2, 1, 0):
                h, w = H >> lvl, W >> lvl
                rows, guard = B * (h + 2) * (w + 2), w + 3
                for _ in range(self.nb):
                    buf = torch.zeros((rows + 2 * guard, self.nc[lvl]), dtype=torch.bfloat16, device=device)
                    grids.append((buf[guard:], h, w, buf))
            self._tapes_by_shape[key] = grids
        return self._tapes_by_shape[key]

    def _blocks16(self, wts, prefix, first, lvl, B, H, W, lv, t_in, last_skip, tape=None):
        """nb ResBlocks `prefix.{first ..}` on level lvl; the trunk starts in t_in and ends in the level's working trunk,
        the last block adds last_skip (the U-Net skip ahead of an up block) when given. With a tape every block's ReLU output
        goes to the tape's next grid instead of the level's shared one."""
        ya, yb, t, _ = lv[lvl][:4]
        c, h, w = self.nc[lvl], H >> lvl, W >> lvl
        for i in range(self.nb):
            skip = last_skip if i == self.nb - 1 else None
            if tape is not None:
                tape.mids.append(tape.grids[len(tape.mids)][:3])
                yb = tape.mids[-1][0]
            N.call("sei_drunet_conv3x3", ya.data_ptr(), wts[f"{prefix}.{first + i}.res.0.weight"].data_ptr(), c, c, B, h, w, 0,
                   None, None, None, yb.data_ptr())
            N.call("sei_drunet_conv3x3", yb.data_ptr(), wts[f"{prefix}.{first + i}.res.2.weight"].data_ptr(), c, c, B, h, w, 1,
                   (t_in if i == 0 else t).data_ptr(), N.ptr(skip), t.data_ptr(), ya.data_ptr())

    def _blocks16_bwd(self, wts, prefix, first, lvl, B, H, W, lv, t_in, last_skip, mids):
        """The backward of _blocks16: the blocks in reverse, G_in = G_out + conv1^T([mid > 0] conv2^T(G_out)); the gradient
        starts in t_in and ends in the level's working trunk, the block reached last adds last_skip (the gradient the U-Net
        skip carries to this stage's input) when given. `mids` yields the taped grids in reverse network order."""
        ya, yb, t, _ = lv[lvl][:4]
        c, h, w = self.nc[lvl], H >> lvl, W >> lvl
        for i in reversed(range(self.nb)):
            N.call("sei_drunet_conv3x3_masked", ya.data_ptr(), wts[f"{prefix}.{first + i}.res.2.weight"].data_ptr(), c, c, B, h,
                   w, next(mids)[0].data_ptr(), yb.data_ptr())
            N.call("sei_drunet_conv3x3", yb.data_ptr(), wts[f"{prefix}.{first + i}.res.0.weight"].data_ptr(), c, c, B, h, w, 1,
                   (t_in if i == self.nb - 1 else t).data_ptr(), N.ptr(last_skip if i == 0 else None), t.data_ptr(),
                   ya.data_ptr())

    def _vjp_bf16(self, tape, g):
        B, _, H, W = g.shape
        wts = self._weights_t("bf16")
        lv, work = self._grids(B, H, W, g.device)
        nc, nb, mids = self.nc, self.nb, reversed(tape.mids)
        # the gradient of x + x1 -- of m_up1's output and of the skip x1: the level's skip buffer keeps it, as below
        N.call("sei_drunet_head", g.data_ptr(), 0.0, wts["m_tail.weight"].data_ptr(), nc[0], B, H, W, lv[0][3].data_ptr(),
               lv[0][0].data_ptr(), work.data_ptr())
        for lvl in (1, 2, 3):
            self._blocks16_bwd(wts, f"m_up{lvl}", 1, lvl - 1, B, H, W, lv, lv[lvl - 1][3], None, mids)
            N.call("sei_drunet_down", lv[lvl - 1][0].data_ptr(), wts[f"m_up{lvl}.0.weight"].data_ptr(), nc[lvl - 1], nc[lvl], B,
                   H >> lvl, W >> lvl, lv[lvl][3].data_ptr(), lv[lvl][0].data_ptr())
        self._blocks16_bwd(wts, "m_body", 0, 3, B, H, W, lv, lv[3][3], lv[3][3], mids)
        for lvl in (3, 2, 1):
            N.call("sei_drunet_up", lv[lvl][0].data_ptr(), wts[f"m_down{lvl}.{nb}.weight"].data_ptr(), nc[lvl], nc[lvl - 1], B,
                   H >> lvl, W >> lvl, lv[lvl - 1][2].data_ptr(), lv[lvl - 1][0].data_ptr())
            self._blocks16_bwd(wts, f"m_down{lvl}", 0, lvl - 1, B, H, W, lv, lv[lvl - 1][2], lv[lvl - 1][3], mids)
        gx = torch.empty_like(g)
        N.call("sei_drunet_tail", lv[0][0].data_ptr(), wts["m_head.weight"].data_ptr(), nc[0], B, H, W, gx.data_ptr())
        return gx

    def _run_bf16(self, x, sigma, tape=None):
        B, _, H, W = x.shape
        wts = self._weights("bf16")
        lv, work = self._grids(B, H, W, x.device)
        nc, nb = self.nc, self.nb
        if tape is not None:
            tape.grids = self._tape_grids(B, H, W, x.device)
        N.call("sei_drunet_head", x.data_ptr(), sigma, wts["m_head.weight"].data_ptr(), nc[0], B, H, W, lv[0][3].data_ptr(),
               lv[0][0].data_ptr(), work.data_ptr())
        for lvl in range(3):
            self._blocks16(wts, f"m_down{lvl + 1}", 0, lvl, B, H, W, lv, lv[lvl][3], None, tape)
            N.call("sei_drunet_down", lv[lvl][0].data_ptr(), wts[f"m_down{lvl + 1}.{nb}.weight"].data_ptr(), nc[lvl],
                   nc[lvl + 1], B, H >> (lvl + 1), W >> (lvl + 1), lv[lvl + 1][3].data_ptr(), lv[lvl + 1][0].data_ptr())
        self._blocks16(wts, "m_body", 0, 3, B, H, W, lv, lv[3][3], lv[3][3], tape)
        for lvl in (3, 2, 1):
            N.call("sei_drunet_up", lv[lvl][0].data_ptr(), wts[f"m_up{lvl}.0.weight"].data_ptr(), nc[lvl], nc[lvl - 1], B,
                   H >> lvl, W >> lvl, lv[lvl - 1][2].data_ptr(), lv[lvl - 1][0].data_ptr())
            self._blocks16(wts, f"m_up{lvl}", 1, lvl - 1, B, H, W, lv, lv[lvl - 1][2], lv[lvl - 1][3], tape)
        out = torch.empty_like(x)
        N.call("sei_drunet_tail", lv[0][0].data_ptr(), wts["m_tail.weight"].data_ptr(), nc[0], B, H, W, out.data_ptr())
        return out

    # "f32": the parity mode, from existing float32 entry points (activations NHWC)
    @staticmethod
    def _gemm32(a, b, d, m, n, k, accumulate):
        N.call("sei_gemm_f32_ex", a.data_ptr(), b.data_ptr(), d.data_ptr(), m, n, k, 0, 1, 5 if accumulate else 0, None, None,
               None, None, 1, 0, 0, 0, 0)

    def _conv32(self, x, wt, res=None):
        """conv3x3 of NHWC x with the per-tap matrices wt (9, Cout, Cin), + res."""
        B, H, W, cin = x.shape
        cout, wp, rows = wt.shape[1], W + 2, B * (H + 2) * (W + 2)
        guard = wp + 1
        xp = torch.empty((rows + 2 * guard, cin), dtype=torch.float32, device=x.device)
        N.call("sei_pad_nhwc", x.data_ptr(), xp.data_ptr(), B, H, W, cin, guard)
        outp = torch.empty((rows, cout), dtype=torch.float32, device=x.device)
        for t, (ky, kx) in enumerate(_TAPS):
            off = guard + (ky - 1) * wp + (kx - 1)
            self._gemm32(xp[off:off + rows], wt[t], outp, rows, cout, cin, t > 0)
        y = torch.empty((B, H, W, cout), dtype=torch.float32, device=x.device)
        N.call("sei_unpad_nhwc", outp.data_ptr(), N.ptr(res), y.data_ptr(), B, H, W, cout, 0)
        return y

    def _blocks32(self, wts, prefix, first, x, tape=None):
        for i in range(self.nb):
            mid = self._conv32(x, wts[f"{prefix}.{first + i}.res.0.weight"]).relu_()
            if tape is not None:
                tape.mids.append(mid)
            x = self._conv32(mid, wts[f"{prefix}.{first + i}.res.2.weight"], x)
        return x

    def _blocks32_bwd(self, wts, prefix, first, g, mids):
        for i in reversed(range(self.nb)):
            gm = self._conv32(g, wts[f"{prefix}.{first + i}.res.2.weight"]) * (next(mids) > 0)
            g = self._conv32(gm, wts[f"{prefix}.{first + i}.res.0.weight"], g)
        return g

    def _vjp_f32(self, tape, g):
        B, _, H, W = g.shape
        wts = self._weights_t("f32")
        nc, nb, mids = self.nc, self.nb, reversed(tape.mids)
        t = torch.empty((B, H, W, nc[0]), dtype=torch.float32, device=g.device)
        N.call("sei_conv3x3_fwd", g.data_ptr(), wts["m_tail.weight"].data_ptr(), None, None, t.data_ptr(), B, H, W, 3, nc[0],
               1, 0, 1)
        skips = [t]                                           # the gradient each U-Net skip carries, by level
        for lvl in (1, 2, 3):
            t = self._blocks32_bwd(wts, f"m_up{lvl}", 1, t, mids)
            h, w, co = t.shape[1] // 2, t.shape[2] // 2, t.shape[3]
            quad = t.view(B, h, 2, w, 2, co).permute(0, 1, 3, 2, 4, 5).reshape(B * h * w, 4 * co)
            t = torch.empty((B, h, w, nc[lvl]), dtype=torch.float32, device=g.device)
            self._gemm32(quad, wts[f"m_up{lvl}.0.weight"], t, B * h * w, nc[lvl], 4 * co, False)
            skips.append(t)
        t = self._blocks32_bwd(wts, "m_body", 0, t, mids) + skips[3]
        for lvl in (3, 2, 1):
            _, h, w, c = t.shape
            ci = nc[lvl - 1]
            taps = torch.empty((B * h * w, 4 * ci), dtype=torch.float32, device=g.device)
            self._gemm32(t.contiguous(), wts[f"m_down{lvl}.{nb}.weight"], taps, B * h * w, 4 * ci, c, False)
            t = taps.view(B, h, w, 2, 2, ci).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * h, 2 * w, ci)
            t = self._blocks32_bwd(wts, f"m_down{lvl}", 0, t, mids) + skips[lvl - 1]
        t = t.contiguous()
        gx = torch.empty_like(g)
        N.call("sei_conv3x3_fwd", t.data_ptr(), wts["m_head.weight"].data_ptr(), None, None, gx.data_ptr(), B, H, W, nc[0], 3,
               0, 1, 1)
        return gx

    def _run_f32(self, x, sigma, tape=None):
        B, _, H, W = x.shape
        wts = self._weights("f32")
        nc, nb = self.nc, self.nb
        x0 = torch.cat([x, torch.full((B, 1, H, W), sigma, dtype=torch.float32, device=x.device)], 1).contiguous()
        x1 = torch.empty((B, H, W, nc[0]), dtype=torch.float32, device=x.device)
        N.call("sei_conv3x3_fwd", x0.data_ptr(), wts["m_head.weight"].data_ptr(), None, None, x1.data_ptr(), B, H, W, 4, nc[0],
               1, 0, 0)
        skips, t = [x1], x1
        for lvl in range(3):
            t = self._blocks32(wts, f"m_down{lvl + 1}", 0, t, tape)
            h, w, c = t.shape[1] // 2, t.shape[2] // 2, t.shape[3]
            taps = t.view(B, h, 2, w, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(B * h * w, 4 * c)
            down = torch.empty((B, h, w, nc[lvl + 1]), dtype=torch.float32, device=x.device)
            self._gemm32(taps, wts[f"m_down{lvl + 1}.{nb}.weight"], down, B * h * w, nc[lvl + 1], 4 * c, False)
            skips.append(down)
            t = down
        t = self._blocks32(wts, "m_body", 0, t, tape)
        for lvl in (3, 2, 1):
            t = t + skips[lvl]
            _, h, w, c = t.shape
            co = nc[lvl - 1]
            quad = torch.empty((B * h * w, 4 * co), dtype=torch.float32, device=x.device)
            self._gemm32(t, wts[f"m_up{lvl}.0.weight"], quad, B * h * w, 4 * co, c, False)
            t = quad.view(B, h, w, 2, 2, co).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * h, 2 * w, co)
            t = self._blocks32(wts, f"m_up{lvl}", 1, t, tape)
        t = (t + skips[0]).contiguous()
        out = torch.empty_like(x)
        N.call("sei_conv3x3_fwd", t.data_ptr(), wts["m_tail.weight"].data_ptr(), None, None, out.data_ptr(), B, H, W, nc[0], 3,
               0, 1, 0)
        return out
