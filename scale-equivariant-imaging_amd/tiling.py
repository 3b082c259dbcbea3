"""Tiled inference (build-side addition): run a feed-forward model on overlapping tiles of an image of any size
and blend the results, so peak memory follows the tile, not the image, and one large image becomes batches of tiles.

The plan of an axis of length n with tile T and overlap v (0 <= 2 v <= T): n <= T gives one tile of extent Te = n at origin
0; otherwise Te = T, the stride is s = T - v, and the origins are 0, s, 2s, ... strictly below n - T followed by n - T: the last
tile is shifted back to end on the border, as the test script of SwinIR does, and nothing is ever padded. Tiles of an image are
the product grid of its two axes, numbered row-major. Window weight of position i inside a tile at origin o:

  uniform   1
  feather   min(i + 1, Te - i, max(v, 1))                                                        (the default)
  crop      1 if lo <= i < Te - hi else 0;  lo = 0 if o == 0 else v // 2;  hi = 0 if o + Te == n else v - v // 2

and out[c, y, x] = (sum over the covering tiles, in tile order, of wy wx tile[c, y - oy, x - ox]) / (Sy(y) Sx(x)), Sy and Sx
the per-axis weight sums. The weights are integers, so their sums and products are exact in float32 (which is why T <= 2048).
`crop` takes every pixel from tiles that see at least v // 2 pixels of context around it: it reproduces the whole-image result
only for a model whose receptive field fits in v // 2. Neither network of this build does (the U-Net's ideal resamplers are
global, SwinIR's 36 shifted-window blocks reach far): for them tiling is an approximation whose seams the overlap hides. No
parity with SwinIR's script is claimed: the script is not in this tree, and `uniform` is its rule restated.

The cut and the blend run in sei_tile_gather and sei_tile_blend (include/sei_hip.h). This module is host arithmetic, the one
definition of the plan every layer uses, and the class that drives the two kernels around a model.
"""
import torch

import _native as N

WINDOWS = ("uniform", "feather", "crop")
MAX_TILE = 2048


def tile_plan(n, T, v):
    """(origins, Te, stride) of one axis. On a single-tile axis the stride places nothing: it carries the overlap that caps
    the feather window, Te - min(v, Te - 1), so that (n, Te, stride, 1) says everything the kernels need there too."""
    n, T, v = int(n), int(T), int(v)
    if n < 1 or T < 1 or v < 0 or 2 * v > T:
        raise ValueError(f"tile_plan: need n >= 1, T >= 1 and 0 <= 2 v <= T, got n = {n}, T = {T}, v = {v}")
    if n <= T:
        return [0], n, n - min(v, n - 1)
    s = T - v
    return list(range(0, n - T, s)) + [n - T], T, s


def axis_weights(kind, n, Te, stride, origin):
    """The integer window weights of the Te positions of the tile at `origin` on an axis of length n (a list)."""
    if kind not in WINDOWS:
        raise ValueError(f"axis_weights: window must be one of {WINDOWS}, got {kind!r}")
    v = Te - stride
    if kind == "uniform":
        return [1] * Te
    if kind == "feather":
        return [min(i + 1, Te - i, max(v, 1)) for i in range(Te)]
    lo = 0 if origin == 0 else v // 2
    hi = 0 if origin + Te == n else v - v // 2
    return [int(lo <= i < Te - hi) for i in range(Te)]


class TiledModel:
    """model(y) on overlapping tiles: y (B, C, H, W) or (C, H, W) on the GPU -> the blended (.., C', scale H, scale W).

    tile, overlap: T and v of the plan, in input pixels, for both axes; batch: tiles per model call; scale: the integer by
    which `model` multiplies the extents (the rate of an SR model); window: one of WINDOWS. `model` is called under
    torch.no_grad() on contiguous float32 (n, C, Th, Tw) batches, n <= batch, and must be feed-forward: a model that carries
    the physics at the whole image's extents (the iterative baselines) would be a different algorithm tile by tile. The images
    of a batch are handled one after another. The gathered tiles live in a buffer that is cached per (C, H, W, plan)."""

    def __init__(self, model, tile, overlap=32, batch=8, scale=1, window="feather"):
        tile, overlap, batch, scale = int(tile), int(overlap), int(batch), int(scale)
        if not 1 <= tile <= MAX_TILE:
            raise ValueError(f"TiledModel: tile must lie in 1 .. {MAX_TILE}, got {tile}")
        if overlap < 0 or 2 * overlap > tile:
            raise ValueError(f"TiledModel: need 0 <= 2 overlap <= tile, got overlap = {overlap}, tile = {tile}")
        if batch < 1 or scale < 1 or scale * tile > MAX_TILE:
            raise ValueError(f"TiledModel: need batch >= 1, scale >= 1 and scale * tile <= {MAX_TILE}, got batch = {batch}, "
                             f"scale = {scale}, tile = {tile}")
        if window not in WINDOWS:
            raise ValueError(f"TiledModel: window must be one of {WINDOWS}, got {window!r}")
        self.model, self.tile, self.overlap, self.batch, self.scale = model, tile, overlap, batch, scale
        self.window = WINDOWS.index(window)
        self._buffers = {}

    def _tiles_buffer(self, key, shape, device):
        buf = self._buffers.get(key)
        if buf is None or buf.device != device:
            self._buffers.clear()                          # one image size at a time: the cache does not grow with a folder
            buf = self._buffers[key] = torch.empty(shape, dtype=torch.float32, device=device)
        return buf

    def _one(self, x):
        C, H, W = x.shape
        (oy, Th, sy), (ox, Tw, sx) = tile_plan(H, self.tile, self.overlap), tile_plan(W, self.tile, self.overlap)
        ny, nx, r = len(oy), len(ox), self.scale
        # the plan of the model's output: the plan times r, which is the canonical plan of the image times r
        (_, rTh, rsy), (_, rTw, rsx) = tile_plan(r * H, r * self.tile, r * self.overlap), \
            tile_plan(r * W, r * self.tile, r * self.overlap)
        total, cap = ny * nx, min(self.batch, ny * nx)
        tiles = self._tiles_buffer((C, H, W, Th, Tw, sy, sx, cap), (cap, C, Th, Tw), x.device)
        out = None
        for t0 in range(0, total, cap):
            n = min(cap, total - t0)
            N.call("sei_tile_gather", x.data_ptr(), tiles.data_ptr(), C, H, W, Th, Tw, sy, sx, ny, nx, t0, n)
            rec = self.model(tiles[:n])
            if rec.dim() != 4 or rec.shape[0] != n or tuple(rec.shape[2:]) != (r * Th, r * Tw):
                raise ValueError(f"TiledModel: the model returned {tuple(rec.shape)} for {n} tiles of extents ({Th}, {Tw}), "
                                 f"expected extents ({r * Th}, {r * Tw}) (scale {r}). A U-Net whose input needs padding to a "
                                 "multiple of 16 keeps extra rows in super-resolution: pick an image or tile extent that is "
                                 "a multiple of 16")
            rec = N.check_tensor(rec.detach().contiguous(), "model output")
            if out is None:
                out = torch.empty((rec.shape[1], r * H, r * W), dtype=torch.float32, device=x.device)
            elif rec.shape[1] != out.shape[0]:
                raise ValueError(f"TiledModel: the model returned {rec.shape[1]} channels after {out.shape[0]}")
            N.call("sei_tile_blend", rec.data_ptr(), out.data_ptr(), out.shape[0], r * H, r * W, rTh, rTw, rsy, rsx, ny, nx,
                   self.window, t0, n, int(t0 > 0), int(t0 + n == total))
        return out

    def __call__(self, y):
        if not isinstance(y, torch.Tensor) or y.dim() not in (3, 4):
            raise ValueError("TiledModel: expected a (B, C, H, W) or (C, H, W) tensor, got "
                             f"{tuple(y.shape) if isinstance(y, torch.Tensor) else type(y).__name__}")
        y = N.check_tensor(y.detach().contiguous(), "y")
        with torch.no_grad():
            if y.dim() == 3:
                return self._one(y)
            first = self._one(y[0])
            if y.shape[0] == 1:
                return first[None]
            out = torch.empty((y.shape[0],) + tuple(first.shape), dtype=torch.float32, device=y.device)
            out[0] = first
            for b in range(1, y.shape[0]):
                out[b] = self._one(y[b])
            return out
