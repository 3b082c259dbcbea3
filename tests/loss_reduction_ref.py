"""CPU references of the loss reductions and the column sums (tests/test_loss_reductions_gpu.py compares the HIP kernels
with them; tests/test_loss_reduction_ref.py anchors them to the oracle's sure_loss, to F.mse_loss and float64 autograd, to
metrics.luma and to (w[:, None] * X).sum(0) on the CPU first):

  sei_sure_terms / sei_sure_loss   csrc/loss_kernels.hip    `sure`
  sei_mse_terms / sei_mse_loss     csrc/loss_kernels.hip    `mse`
  sei_luma_sqerr                   csrc/loss_kernels.hip    `luma_sqerr`
  sei_colsum_f32 / _weighted_f32   csrc/reduce_kernels.hip  `colsum`

Plain torch on the CPU: nothing of the library under test is imported here. Every reference takes the float32 values the
entry point is handed (the operands, and the scalar arguments rounded to float32 as the C call rounds them) as exact and
evaluates them in `dtype`: torch.float64 is the reference, torch.float32 the identical chain whose deviation is `ref32`.
The float32 chain makes the kernels' element-wise operations one IEEE operation at a time in the kernels' order (the library
is built with -ffp-contract=off), so that

  exact     ga = scale * (a - b) and g2 = (c_div * b) * inv_tau, inv_tau = 1.0f / tau: bit for bit (streaming_ref.same_bits)
  float32   g1, through an explicit fmaf in the kernel: streaming_ref.hold32 at FLOOR
  sums      streaming_ref.hold32_on at FLOOR: deviations relative to the float64 sum of the ABSOLUTE terms, which every
            reference returns beside the sum. (The divergence sum cancels to about 1e-3 of that scale on random data: a
            bar relative to the sum itself would test the inputs, not the kernel.) The loss value uses the scale
            |c_mse| S_mse + |c_div| S|div| + |cst|.
  columns   streaming_ref.hold32 at REDUCTION_FLOOR, relative to the largest column of the float64 result

The cases are drawn here, once per process (the draws and the float64 references are cached and must not be written to),
so that the CPU module measures `ref32` on exactly what the GPU module feeds the kernels. MEASURED_REF32 records those
values as tests/test_loss_reduction_ref.py prints them: all below a third of the floors, so the floors are the bars.
"""
import functools

import torch

SIGMA = 0.1                  # noise level of the SURE constants (c_div = 2 sigma^2 / n_div, cst = sigma^2 / B)
TAU = 0.01                   # losses/sure.py's default probe step

# ref32 of the families on the drawn cases as tests/test_loss_reduction_ref.py prints them (largest over the cases)
# (the one- and few-element cases set them: a single rounding there is the whole deviation; past 10^5 elements the two SURE
# sums sit at 3e-10 .. 5e-8 of their scales)
MEASURED_REF32 = {"sure div": 8.0e-8, "sure mse": 1.2e-7, "sure loss": 8.0e-8, "sure g1": 1.1e-7, "mse sum": 8.6e-8,
                  "mse value": 1.2e-7, "luma sqerr": 7.2e-7, "column sums": 5.7e-7, "weighted column sums": 1.8e-7}

# ---------------------------------------------------------------------------------------------- cases
# (planes, H, W, margin_div, margin_mse): the smallest at which each path of sure_terms_kernel exists. A two-stage
# reduction launches min(256, ceil(n / 1024)) workgroups of 256 threads: up to n = 262144 a thread handles at most 4
# elements, past it the grid-stride loop does the work.
SURE_GRID = [
    (1, 1, 1, 0, 0),             # one element
    (1, 5, 9, 1, 2),             # non-square, W > H, the mse margin the larger
    (1, 9, 5, 2, 1),             # non-square, H > W, the divergence margin the larger
    (2, 7, 7, 3, 3),             # a one-pixel interior
    (2, 8, 8, 3, 0),             # a 2 x 2 divergence interior inside a full mse interior
    (5, 3, 17, 0, 1),            # 255 elements: one partly idle workgroup
    (1, 16, 16, 0, 0),           # 256
    (1, 257, 1, 0, 0),           # a one-column image
    (3, 48, 48, 6, 6),           # the product's two forms: cropped divergence ...
    (3, 48, 48, 0, 6),           # ... and uncropped
    (4, 256, 256, 0, 0),         # 262144: the cap reached exactly
    (7, 200, 190, 6, 3),         # 266000: just past the cap, a ragged last sweep
    (9, 256, 261, 2, 5),         # 601344: nine sweeps and a ragged tenth
]
# the grid with border_b: in every second case b is NONZERO on the margin_div-wide border (of the seven cases with a
# divergence margin, three), so that the kernel's masks, not b's zeros, do the cropping
SURE_CASES = [case + (i % 2 == 1,) for i, case in enumerate(SURE_GRID)]
SURE_TERMS_SUBSET = [SURE_CASES[i] for i in (0, 1, 2, 3, 9, 10, 11)]         # also run through sei_sure_terms
SURE_NEGATIVE_TAU = (1, 5, 9, 1, 2, True)
SURE_JOINT = (3, 48, 48, 6, 6, False)
SURE_OFFSET = (7, 200, 190, 6, 3, True)
CAP = 262144                 # elements of one sweep of the capped grid (256 workgroups x 256 threads x 4)

MSE_N = [1, 3, 255, 256, 257, 1023, 1024, 1025, CAP, CAP + 1, 600001]
MSE_SCALES = ["w=1", "w=0.1", "dip"]
LUMA_NPIX = [1, 255, 257, 1025, CAP, CAP + 3, 600001]
PSNR_IMAGE = (3, 531, 497)   # 263907 pixels: non-square and past the cap

# (M, N) whose rows are float4-able: colsum_vec_kernel when X is 16-byte aligned
COLSUM_VEC = [
    (1, 4), (255, 4), (2049, 4),         # tpr 1; M below, at and just past one 8-sweep pass (256 rows x 8); a one-row tail
    (37, 12), (2049, 12),                # 3 quads on 4 lanes: one dead lane
    (333, 100),                          # 25 quads on 32 lanes (100 % 4 == 0: aligned, this is no scalar-kernel shape)
    (5000, 300),                         # 75 quads on 128 lanes; rows_per_block doubling; a ragged last row block
    (17, 1024), (300, 1028),             # tpr 256; a second column block with one live quad
    (288, 8192), (73728, 32),            # the shapes the network uses
]
# colsum_kernel: N % 4 != 0
COLSUM_SCALAR = [
    (50, 1), (50, 3), (40000, 7),        # narrow widths
    (100, 255),                          # one idle thread
    (64, 257),                           # a second column block with one live column
]
# N % 4 == 0 on an unaligned pointer: the dispatch falls back to colsum_kernel. (333, 100) there is that kernel's
# rsubs = 2 with 56 idle threads (256 % N != 0)
COLSUM_UNALIGNED = [(1000, 128), (300, 1028), (333, 100)]


def f32(v):
    """A Python float as the C call rounds it to its `float` argument."""
    return torch.tensor(float(v), dtype=torch.float32)


def scalar(v, dtype, rounded=True):
    """The scalar argument `v` in `dtype`: through float32, as the kernel receives it, or (rounded=False, for the anchors
    to formulas that never round it) as it is."""
    return f32(v).to(dtype) if rounded else torch.tensor(float(v), dtype=dtype)


def _gen(*key):
    """A generator seeded from a case's integers."""
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- SURE
def interior(H, W, m):
    """True on [m : H - m, m : W - m] of an H x W image."""
    mask = torch.zeros((H, W), dtype=torch.bool)
    mask[m:H - m, m:W - m] = True
    return mask


def sure_constants(planes, H, W, md, mm, sigma=SIGMA):
    """(c_mse, c_div, cst) as losses/sure.py forms them, for `planes` one-channel images."""
    n_div, n_mse = planes * (H - 2 * md) * (W - 2 * md), planes * (H - 2 * mm) * (W - 2 * mm)
    return 1.0 / n_mse, 2.0 * sigma ** 2 / n_div, sigma ** 2 / planes


@functools.lru_cache(maxsize=None)
def sure_inputs(planes, H, W, md, mm, border_b):
    """y, y1, y2, b of shape (planes, H, W) in float32. y in [0, 1], y1 = y + noise, y2 = y1 + tau * O(1) (what a model
    returns for the probe y + tau b), b ~ N(0, 1). border_b False: b is zero on the margin_div-wide border, as
    losses/sure.py's draw_probe leaves it; True: b is nonzero there, and only the kernel's masks crop."""
    gen = _gen(planes, H, W, md, mm)
    y = torch.rand((planes, H, W), generator=gen)
    y1 = y + 0.1 * torch.randn((planes, H, W), generator=gen)
    y2 = y1 + TAU * torch.randn((planes, H, W), generator=gen)
    b = torch.randn((planes, H, W), generator=gen)
    b[b == 0] = 1.0
    if not border_b:
        b = torch.where(interior(H, W, md), b, torch.zeros(()))
    return y, y1, y2, b


def sure(y, y1, y2, b, md, mm, tau, c_mse, c_div, cst, dtype, rounded=True):
    """What sei_sure_loss is to return: a dict of
        div, mse     out3[0] = sum over the margin_div interior of b (y2 - y1) / tau, out3[1] = sum over the margin_mse
                     interior of (y1 - y)^2
        loss         out3[2] = c_mse mse + c_div div - cst
        abs_div      the sum of |b (y2 - y1) / tau| over the same interior; loss_scale = |c_mse| mse + |c_div| abs_div + |cst|
        g1, g2       2 c_mse (y1 - y) [mse interior] - c_div b / tau [div interior], c_div b / tau [div interior]; 0 outside
    from the float32 operands and the float32-rounded scalars, evaluated in `dtype`. In float32 every element-wise
    operation is the kernel's own, in its order: inv_tau = 1 / tau, (b * (y2 - y1)) * inv_tau, (c_div * b) * inv_tau,
    (2 c_mse) * d + (-gb) (the kernel fuses this last one)."""
    H, W = y.shape[-2:]
    in_d, in_m = interior(H, W, md), interior(H, W, mm)
    y, y1, y2, b = (t.to(dtype) for t in (y, y1, y2, b))
    tau, c_mse, c_div, cst = (scalar(v, dtype, rounded) for v in (tau, c_mse, c_div, cst))
    zero = torch.zeros((), dtype=dtype)
    inv_tau = torch.ones((), dtype=dtype) / tau
    t_div = torch.where(in_d, (b * (y2 - y1)) * inv_tau, zero)
    d = y1 - y
    t_mse = torch.where(in_m, d * d, zero)
    g2 = torch.where(in_d, (c_div * b) * inv_tau, zero)
    ga = torch.where(in_d, -g2, zero)
    g1 = torch.where(in_m, (2 * c_mse) * d + ga, ga)
    div, mse, abs_div = t_div.sum(), t_mse.sum(), t_div.abs().sum()
    return dict(div=div, mse=mse, abs_div=abs_div, loss=c_mse * mse + c_div * div - cst,
                loss_scale=c_mse.abs() * mse + c_div.abs() * abs_div + cst.abs(), g1=g1, g2=g2)


@functools.lru_cache(maxsize=None)
def sure_case(planes, H, W, md, mm, border_b, tau=TAU):
    """(inputs, constants, float64 reference, float32 chain) of one grid case."""
    inp = sure_inputs(planes, H, W, md, mm, border_b)
    c = sure_constants(planes, H, W, md, mm)
    return inp, c, sure(*inp, md, mm, tau, *c, torch.float64), sure(*inp, md, mm, tau, *c, torch.float32)


# ---------------------------------------------------------------------------------------------- mse
def mse_scales(kind, n):
    """(grad_scale, value_scale) as the product's callers form them: losses/ei.py with the EI weight w, models/dip.py."""
    if kind == "dip":
        return 2.0 / n, 1.0 / n
    w = {"w=1": 1.0, "w=0.1": 0.1}[kind]
    return 2.0 * w / n, w / n


@functools.lru_cache(maxsize=None)
def mse_inputs(n):
    gen = _gen(n, 17)
    a = torch.rand(n, generator=gen)
    return a, a + 0.2 * torch.randn(n, generator=gen)


def mse(a, b, grad_scale, value_scale, dtype, rounded=True):
    """sei_mse_loss: sum = sum (a - b)^2 (all terms positive: its own scale), value = value_scale * sum,
    ga = grad_scale * (a - b); in float32 one subtract and one multiply per element, as the kernel makes them."""
    a, b = a.to(dtype), b.to(dtype)
    gs, vs = scalar(grad_scale, dtype, rounded), scalar(value_scale, dtype, rounded)
    d = a - b
    total = (d * d).sum()
    return dict(sum=total, value=vs * total, ga=gs * d)


# ---------------------------------------------------------------------------------------------- luma
LUMA_COEF = (0.299, 0.587, 0.114)


@functools.lru_cache(maxsize=None)
def luma_inputs(npix):
    """Two planar RGB images (3, npix) in [0, 1]."""
    gen = _gen(npix, 23)
    return torch.rand((3, npix), generator=gen), torch.rand((3, npix), generator=gen)


def luma_of(img, dtype):
    """Y = 0.299 R + 0.587 G + 0.114 B of a planar (3, ...) image with the coefficients as float32 constants (the kernel's
    0.299f, 0.587f, 0.114f), summed left to right."""
    c = [f32(v).to(dtype) for v in LUMA_COEF]
    img = img.to(dtype)
    return c[0] * img[0] + c[1] * img[1] + c[2] * img[2]


def luma_sqerr(a, b, dtype):
    """sei_luma_sqerr: sum over the pixels of (Y(a) - Y(b))^2."""
    d = luma_of(a, dtype) - luma_of(b, dtype)
    return (d * d).sum()


@functools.lru_cache(maxsize=None)
def psnr_images():
    """A clean image in [0, 1] and a noisy estimate of it, shape PSNR_IMAGE."""
    gen = _gen(*PSNR_IMAGE)
    x = torch.rand(PSNR_IMAGE, generator=gen)
    return (x + 0.05 * torch.randn(PSNR_IMAGE, generator=gen)).clamp(0, 1), x


def psnr_db(x_hat, x, dtype):
    """10 log10(1 / mean (Y(x_hat) - Y(x))^2) for (3, H, W) images."""
    npix = x.shape[-2] * x.shape[-1]
    return 10.0 * torch.log10(1.0 / (luma_sqerr(x_hat.reshape(3, -1), x.reshape(3, -1), dtype) / npix))


# ---------------------------------------------------------------------------------------------- column sums
@functools.lru_cache(maxsize=None)
def colsum_inputs(M, N):
    """X (M, N), signed row weights with exact zeros among them (about one in eight; the first row's where M > 1), and the
    random values the destination holds before the call: the entry points ADD to it."""
    gen = _gen(M, N, 29)
    X = torch.randn((M, N), generator=gen)
    w = torch.randn(M, generator=gen)
    w[torch.rand(M, generator=gen) < 0.125] = 0.0
    if M > 1:
        w[0] = 0.0
    return X, w, torch.randn(N, generator=gen)


def colsum(X, w, out0, dtype):
    """out0[n] + sum_m w[m] X[m, n] (w None: the plain sums)."""
    X = X.to(dtype)
    rows = X if w is None else w.to(dtype)[:, None] * X
    return out0.to(dtype) + rows.sum(0)


def colsum_row_blocks(M, N, aligned):
    """The number of row blocks launch_colsum (csrc/reduce_kernels.hip) tiles M into. With one, every column receives a
    single atomic add and the result does not depend on the order in which workgroups retire."""
    ceil_div = lambda a, b: (a + b - 1) // b
    if N % 4 == 0 and aligned:
        quads, tpr = N // 4, 1
        while tpr < quads and tpr < 256:
            tpr *= 2
        col_blocks, rpb, most = ceil_div(quads, tpr), (256 // tpr) * 8, 128
    else:
        col_blocks, rpb, most = ceil_div(N, min(N, 256)), 16, 2048
    while ceil_div(M, rpb) * col_blocks > most and rpb < M:
        rpb *= 2
    return ceil_div(M, rpb)
