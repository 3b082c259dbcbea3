"""The order in which the library folds per-workgroup partial sums into a gradient, as numpy float32.

Every reducing kernel of the backward passes leaves partial sums `part[groups][ncol]`; a second stage (csrc/reduce_kernels.hip:
`fold_entries`, run by `sei_fold_many` and by every entry point that is handed its destinations) adds them to the running
gradient without atomics, in ONE fixed order. This module states that order independently of the kernels, so that a test
can hold them to it bit for bit: the library is built with -ffp-contract=off and without fast-math, hence elementwise
float32 additions in numpy are exactly the additions the kernels make. (The float4 schedule of `fold_many_kernel` loads
differently and adds in this same order.)

Test infrastructure, like the rest of `oracle/`: nothing under the product package imports it.
"""
import numpy as np

SLICES = 16          # a column's groups are dealt to 16 interleaved slices: slice k owns groups k, k + 16, k + 32, ...
CHAINS = 4           # a slice keeps four independent sums while it has four groups left

FOLD_SPLIT, FOLD_DWCONV7 = 0, 1      # SEI_FOLD_SPLIT, SEI_FOLD_DWCONV7 of include/sei_hip.h


def fold_segment(part):
    """(groups, ncol) float32 -> (ncol,) float32: the sum over the groups in the kernels' order."""
    part = np.asarray(part)
    assert part.dtype == np.float32 and part.ndim == 2
    groups, ncol = part.shape
    total = np.zeros(ncol, np.float32)
    for k in range(SLICES):
        s = [np.zeros(ncol, np.float32) for _ in range(CHAINS)]
        p = k
        while p + (CHAINS - 1) * SLICES < groups:            # four chains, SLICES groups apart
            for j in range(CHAINS):
                s[j] = s[j] + part[p + SLICES * j]
            p += CHAINS * SLICES
        while p < groups:                                    # the tail goes to chain 0
            s[0] = s[0] + part[p]
            p += SLICES
        total = total + ((s[0] + s[1]) + (s[2] + s[3]))      # the slices meet in slice order, from 0
    return total


def fold_job(kind, split, segments, a, b=None, c=None):
    """A SeiFoldJob: the segments (arrays (groups, ncol), one per launch that feeds the destination) are folded one after
    the other into the running value, dst + t0 + t1 + ..., and entry e of the ncol lands
      FOLD_SPLIT:   in a[e] for e < split, b[e - split] for e < 2 split, c[e - 2 split] beyond;
      FOLD_DWCONV7: e = t * split + c, in a[c, t] (a: (split, 49)) for t < 49 and in b[c] for t = 49.
    A destination that is None is dropped. Returns new arrays (a, b, c); the inputs are left alone."""
    ncol = segments[0].shape[1]
    assert 1 <= len(segments) <= 3 and all(s.shape[1] == ncol for s in segments)
    e = np.arange(ncol)
    if kind == FOLD_DWCONV7:
        assert ncol == 50 * split
        t, ch = e // split, e % split
        which, index = np.where(t < 49, 0, 1), np.where(t < 49, ch * 49 + t, ch)
    else:
        assert kind == FOLD_SPLIT and ncol <= 3 * split
        which, index = e // split, e % split
    totals = [fold_segment(seg) for seg in segments]
    outs = [None if d is None else np.array(d, dtype=np.float32) for d in (a, b, c)]
    for k, dst in enumerate(outs):
        if dst is None:
            continue
        flat, sel = dst.reshape(-1), which == k              # (a view: np.array made dst contiguous)
        run = flat[index[sel]]
        for total in totals:
            run = run + total[sel]
        flat[index[sel]] = run
    return tuple(outs)
