"""CPU restatement of tiled inference (tiling.py, sei_tile_gather, sei_tile_blend): plain loops over tiles in
torch, float64 by default and the same chain in float32 for `ref32`. Nothing of the library under test is imported: the plan
and the windows are written out again here, from the definition."""
import torch

WINDOWS = ("uniform", "feather", "crop")


def plan(n, T, v):
    """(origins, Te) of one axis: one tile of extent n where n <= T; otherwise extent T at 0, s, 2s, ... strictly below
    n - T (s = T - v), then n - T."""
    if n <= T:
        return [0], n
    s, origins, o = T - v, [], 0
    while o < n - T:
        origins.append(o)
        o += s
    return origins + [n - T], T


def weights(kind, n, Te, v, o, dtype=torch.float64):
    """The window of the tile at origin o, a (Te,) tensor."""
    i = torch.arange(Te)
    if kind == "uniform":
        w = torch.ones(Te)
    elif kind == "feather":
        w = torch.minimum(torch.minimum(i + 1, Te - i), torch.tensor(max(v, 1)))
    elif kind == "crop":
        lo = 0 if o == 0 else v // 2
        hi = 0 if o + Te == n else v - v // 2
        w = (i >= lo) & (i < Te - hi)
    else:
        raise ValueError(kind)
    return w.to(dtype)


def tiles_of(H, W, T, v):
    """[(oy, ox)] in tile order (row-major over the product grid), and the extents (Th, Tw)."""
    (oy, Th), (ox, Tw) = plan(H, T, v), plan(W, T, v)
    return [(a, b) for a in oy for b in ox], Th, Tw


def gather(x, T, v):
    """(C, H, W) -> the (tiles, C, Th, Tw) batch, by slicing."""
    origins, Th, Tw = tiles_of(x.shape[1], x.shape[2], T, v)
    return torch.stack([x[:, a:a + Th, b:b + Tw] for a, b in origins])


def blend(tiles, H, W, T, v, kind, scale=1, dtype=torch.float64):
    """(tiles, C, scale Th, scale Tw) -> (C, scale H, scale W): the weighted sum over the tiles in order, over the weight sum
    (the product of the per-axis sums: the 2-D sum factorises). The plan of the scaled image is the plan times `scale`."""
    H, W, T, v = scale * H, scale * W, scale * T, scale * v
    origins, Th, Tw = tiles_of(H, W, T, v)
    assert tuple(tiles.shape[2:]) == (Th, Tw) and tiles.shape[0] == len(origins), (tiles.shape, Th, Tw, len(origins))
    num = torch.zeros((tiles.shape[1], H, W), dtype=dtype)
    sy, sx = torch.zeros(H, dtype=dtype), torch.zeros(W, dtype=dtype)
    for a in plan(H, T, v)[0]:
        sy[a:a + Th] += weights(kind, H, Th, v, a, dtype)
    for b in plan(W, T, v)[0]:
        sx[b:b + Tw] += weights(kind, W, Tw, v, b, dtype)
    for tile, (a, b) in zip(tiles.to(dtype), origins):
        w = weights(kind, H, Th, v, a, dtype)[:, None] * weights(kind, W, Tw, v, b, dtype)[None, :]
        num[:, a:a + Th, b:b + Tw] += w * tile
    return num / (sy[:, None] * sx[None, :])


def coverage(H, W, T, v, kind):
    """(H, W) count of the tiles with non-zero weight per pixel, and the same count over every tile but the shifted last
    row and column of the grid (`regular`)."""
    origins, Th, Tw = tiles_of(H, W, T, v)
    oy, ox = plan(H, T, v)[0], plan(W, T, v)[0]
    count, in_last = torch.zeros((H, W), dtype=torch.int64), torch.zeros((H, W), dtype=torch.bool)
    for a, b in origins:
        w = weights(kind, H, Th, v, a)[:, None] * weights(kind, W, Tw, v, b)[None, :]
        count[a:a + Th, b:b + Tw] += (w != 0).long()
        if (len(oy) > 1 and a == oy[-1]) or (len(ox) > 1 and b == ox[-1]):
            in_last[a:a + Th, b:b + Tw] = True
    return count, in_last


def tiled(model, x, T, v, kind, scale=1, dtype=torch.float64):
    """The whole chain around `model` (a callable on a (tiles, C, Th, Tw) batch)."""
    return blend(model(gather(x.to(dtype), T, v)), x.shape[1], x.shape[2], T, v, kind, scale, dtype)
