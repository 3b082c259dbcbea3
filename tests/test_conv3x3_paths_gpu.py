"""Every kernel behind sei_conv3x3_fwd and sei_conv3x3_bwd_weight, called directly through the C ABI at the shapes that
pick it: the lane-per-channel kernels at each width of the small tensor and in both of its layouts, the pixel-per-thread
kernels, the generic ones, the fallback for misaligned operands, second trips of the grid-stride loops, and the refusal.

Reference: float64 F.conv2d(padding=1) with torch.autograd.grad on the CPU. Every case checks the forward with bias and
residual and once with neither, the transposed call (the data gradient, with the caller's channel roles swapped as
Conv3x3Fn.backward does) and sei_conv3x3_bwd_weight accumulating into non-zero gw and gb. Bars (max-norm relative): 5e-6
for the forward and the data gradient, 2e-5 for the weight and bias gradients -- those of tests/test_unet_gpu.py.
Where float32 F.conv2d on the CPU deviates from float64 by more than a third of a bar, that case's bar is three times
the deviation (the margin of the scale-transform test, for a different summation order). On the small images that never
happens (float32 F.conv2d deviates by at most 5.7e-7 in the forward and the data gradient, 1.1e-6 in the weight and bias
gradients); the long weight-gradient sums of test_second_trips_of_the_grid_stride_loops do, and its docstring has the
figures.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
FWD_BAR, WGRAD_BAR = 5e-6, 2e-5


def relerr(a, b):
    a, b = (t.detach().cpu().double().numpy() for t in (a, b))
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def bar_for(bar, f32_deviation):
    """`bar`, or three times the float32 CPU evaluation's own deviation where that exceeds a third of it."""
    return 3 * f32_deviation if f32_deviation > bar / 3 else bar


def make_case(Ci, Co, B, H, W):
    gen = torch.Generator().manual_seed(1000 * Ci + 10 * Co + B + H + W)
    r = lambda *s: torch.randn(s, generator=gen)
    return dict(x=r(B, Ci, H, W), w=r(Co, Ci, 3, 3) * 0.2, b=r(Co), res=r(B, Co, H, W), gy=r(B, Co, H, W),
                base_w=r(Co, Ci, 3, 3), base_b=r(Co))


def whole_reference(c, dtype=torch.float64):
    """(conv + bias, data gradient, weight gradient, bias gradient) of F.conv2d(padding=1) by torch.autograd, in `dtype`."""
    xr, wr, br = (c[k].to(dtype).requires_grad_(True) for k in ("x", "w", "b"))
    conv = F.conv2d(xr, wr, br, padding=1)
    rgx, rgw, rgb = torch.autograd.grad(conv, [xr, wr, br], c["gy"].to(dtype))
    return conv.detach(), rgx, rgw, rgb


def sample_positions(B, H, W, n=4096):
    """A fixed random sample of n pixels plus all four borders of every image: (image, row, column) index vectors."""
    gen = torch.Generator().manual_seed(4096)
    flat = [torch.randint(0, B * H * W, (n,), generator=gen)]
    img = torch.arange(B)[:, None] * (H * W)
    rows, cols = torch.arange(H) * W, torch.arange(W)
    for edge in (cols, (H - 1) * W + cols, rows, rows + W - 1):
        flat.append((img + edge[None, :]).reshape(-1))
    p = torch.unique(torch.cat(flat))
    return p // (H * W), (p // W) % H, p % W


def sampled_reference(c, pos, dtype=torch.float64):
    """The same four quantities as whole_reference with conv + bias and the data gradient at the pixels `pos` only, as
    (N, channels) matrices: nine matrix products per quantity, one per tap, in `dtype`. The weight and bias gradients are
    whole. (test_sampled_reference_is_the_autograd_one holds this to whole_reference.)"""
    x, w, gy = (c[k].to(dtype) for k in ("x", "w", "gy"))
    B, Ci, H, W = x.shape
    bi, i, j = pos
    xp, gp = F.pad(x, (1, 1, 1, 1)), F.pad(gy, (1, 1, 1, 1))
    conv = c["b"].to(dtype).expand(len(bi), -1).clone()
    rgx = torch.zeros((len(bi), Ci), dtype=dtype)
    rgw = torch.zeros(w.shape, dtype=dtype)
    for ky in range(3):
        for kx in range(3):
            conv += xp[bi, :, i + ky, j + kx] @ w[:, :, ky, kx].T
            rgx += gp[bi, :, i + 2 - ky, j + 2 - kx] @ w[:, :, ky, kx]
            rgw[:, :, ky, kx] = torch.einsum("bohw,bihw->oi", gy, xp[:, :, ky:ky + H, kx:kx + W])
    return conv, rgx, rgw, gy.sum((0, 2, 3))


def at(t, pos):
    """The (N, channels) values of the NCHW tensor `t` at the pixels `pos`."""
    bi, i, j = pos
    return t[bi, :, i, j]


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def lay(t, is_nchw):
    return (t if is_nchw else nhwc(t)).contiguous().cuda()


def canon(t, is_nchw):
    """An image tensor in either layout as an NCHW view on the CPU."""
    t = t.cpu()
    return t if is_nchw else t.permute(0, 3, 1, 2)


def at_offset(t, k, pad=64):
    """A contiguous copy of `t` that starts k floats into a fresh allocation, NaN in front of it and behind it (the views
    of tests/test_dispatch_edges_gpu.py)."""
    base = torch.full((k + t.numel() + pad,), float("nan"), dtype=t.dtype, device="cuda")
    v = base[k:k + t.numel()].view(t.shape)
    v.copy_(t.cuda())
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * k % 16
    return v


def run_kernels(c, nchw_in, nchw_out):
    """The four launches of a case. Returns NCHW views on the CPU: y (bias and residual), y0 (neither), gx, and the
    increments of gw and gb over their non-zero starting values. Outputs start as NaN: an unwritten element fails."""
    import _native as N
    B, Ci, H, W = c["x"].shape
    Co = c["w"].shape[0]
    xd, rd, gyd = lay(c["x"], nchw_in), lay(c["res"], nchw_out), lay(c["gy"], nchw_out)
    wd, bd = c["w"].cuda(), c["b"].cuda()
    y, y0, gx = torch.full_like(rd, float("nan")), torch.full_like(rd, float("nan")), torch.full_like(xd, float("nan"))
    N.call("sei_conv3x3_fwd", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), rd.data_ptr(), y.data_ptr(), B, H, W, Ci, Co,
           int(nchw_in), int(nchw_out), 0)
    N.call("sei_conv3x3_fwd", xd.data_ptr(), wd.data_ptr(), None, None, y0.data_ptr(), B, H, W, Ci, Co,
           int(nchw_in), int(nchw_out), 0)
    N.call("sei_conv3x3_fwd", gyd.data_ptr(), wd.data_ptr(), None, None, gx.data_ptr(), B, H, W, Co, Ci,
           int(nchw_out), int(nchw_in), 1)
    gw, gb = c["base_w"].cuda(), c["base_b"].cuda()
    N.call("sei_conv3x3_bwd_weight", xd.data_ptr(), gyd.data_ptr(), gw.data_ptr(), gb.data_ptr(), B, H, W, Ci, Co,
           int(nchw_in), int(nchw_out))
    torch.cuda.synchronize()
    return (canon(y, nchw_out), canon(y0, nchw_out), canon(gx, nchw_in),
            gw.cpu().double() - c["base_w"].double(), gb.cpu().double() - c["base_b"].double())


def check(Ci, Co, B, H, W, nchw_in, nchw_out, sampled=False, bars=(FWD_BAR, FWD_BAR, WGRAD_BAR, WGRAD_BAR)):
    """One case against float64: bars = (forward, data gradient, weight gradient, bias gradient)."""
    c = make_case(Ci, Co, B, H, W)
    y, y0, gx, dgw, dgb = run_kernels(c, nchw_in, nchw_out)
    if sampled:
        pos = sample_positions(B, H, W)
        conv, rgx, rgw, rgb = sampled_reference(c, pos)
        y, y0, gx, res = at(y, pos), at(y0, pos), at(gx, pos), at(c["res"], pos).double()
        bias = c["b"].double()[None, :]
    else:
        conv, rgx, rgw, rgb = whole_reference(c)
        res, bias = c["res"].double(), c["b"].double()[None, :, None, None]
    errs = (relerr(y, conv + res), relerr(y0, conv - bias), relerr(gx, rgx), relerr(dgw, rgw), relerr(dgb, rgb))
    print(f"conv3x3 {Ci}->{Co} on ({B}, {H}, {W}) nchw_in={int(nchw_in)} nchw_out={int(nchw_out)}: forward {errs[0]:.2e}, "
          f"plain {errs[1]:.2e}, data gradient {errs[2]:.2e}, weight gradient {errs[3]:.2e}, bias gradient {errs[4]:.2e}")
    what = f"{Ci}->{Co} on ({B}, {H}, {W})"
    assert errs[0] < bars[0] and errs[1] < bars[0], (what, "forward", errs[:2])
    assert errs[2] < bars[1], (what, "data gradient", errs[2])
    assert errs[3] < bars[2] and errs[4] < bars[3], (what, "weight / bias gradient", errs[3:])


def test_sampled_reference_is_the_autograd_one():
    """The per-tap matrix products that serve as the reference at sampled pixels of the large images, against float64
    torch.autograd of F.conv2d on a small image, at every pixel (sample and borders cover all of a 3 x 5 x 4 batch)."""
    c = make_case(3, 5, 3, 5, 4)
    pos = sample_positions(3, 5, 4)
    assert len(pos[0]) == 60
    conv, rgx, rgw, rgb = whole_reference(c)
    s_conv, s_rgx, s_rgw, s_rgb = sampled_reference(c, pos)
    assert relerr(s_conv, at(conv, pos)) < 1e-14 and relerr(s_rgx, at(rgx, pos)) < 1e-14
    assert relerr(s_rgw, rgw) < 1e-14 and relerr(s_rgb, rgb) < 1e-14


LANE_IMAGES = [(2, 5, 17), (1, 1, 16), (3, 7, 1), (1, 3, 33), (2, 4, 15)]


@gpu
@pytest.mark.parametrize("nchw_small", [False, True])
@pytest.mark.parametrize("CS", [1, 2, 3, 4])
def test_lane_kernels_hidden_to_small(CS, nchw_small):
    """32 -> CS channels, hidden tensor NHWC, small tensor in either layout. Forward: conv3x3_c32_to_small_kernel<CS> (32
    input channels in NHWC and at most 4 output channels). Transposed call, CS -> 32: conv3x3_small_to_c32_kernel<CS>
    transposed (32 NHWC output channels, at most 4 input channels, y 16-byte aligned). Weight gradient: the MFMA kernel
    for CS <= 3, conv3x3_wgrad_c32_kernel<4, true> for CS = 4 (hidden input NHWC, 4 output channels). Images: a run of 16
    plus a ragged one, a single row of one whole run, one-pixel-wide images, two runs and one pixel, a short run."""
    for B, H, W in LANE_IMAGES:
        check(32, CS, B, H, W, False, nchw_small)


@gpu
@pytest.mark.parametrize("nchw_small", [False, True])
@pytest.mark.parametrize("CS", [1, 2, 3, 4])
def test_lane_kernels_small_to_hidden(CS, nchw_small):
    """CS -> 32 channels, small tensor in either layout, hidden tensor NHWC. Forward: conv3x3_small_to_c32_kernel<CS> (32
    NHWC output channels, at most 4 input channels, y / res / bias 16-byte aligned). Transposed call, 32 -> CS:
    conv3x3_c32_to_small_kernel<CS> transposed. Weight gradient: the MFMA kernel for CS <= 3,
    conv3x3_wgrad_c32_kernel<4, false> for CS = 4 (hidden output gradient NHWC, 4 input channels). Same images."""
    for B, H, W in LANE_IMAGES:
        check(CS, 32, B, H, W, nchw_small, False)


@gpu
@pytest.mark.parametrize("nchw_in,nchw_out", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("Ci,Co", [(64, 3), (16, 3), (3, 16), (8, 32), (5, 8)])
def test_pixel_per_thread_kernels(Ci, Co, nchw_in, nchw_out):
    """Shapes outside the lane kernels (no 32-channel NHWC tensor beside one of at most 4 channels) with 3, 8, 16 or 32
    output channels: conv3x3_pix_kernel<Cout>, on (2, 9, 13), NHWC throughout and with either end NCHW.
      64 -> 3 (SwinIR conv_last, DRUNet tail): pix<3>; transposed 3 -> 64: the generic kernel transposed (64 outputs);
                weight gradient tiled with P = 16 (3 + 576 floats per pixel in 48 KiB)
      16 -> 3:  pix<3>; transposed pix<16>; weight gradient tiled, P = 64 (3 + 144 floats per pixel)
      3 -> 16:  pix<16>; transposed pix<3>; weight gradient tiled, P = 128
      8 -> 32:  pix<32> (8 input channels: not a lane shape); transposed 32 -> 8: pix<8>; weight gradient generic
                (32 * 72 = 2304 outputs > 2048)
      5 -> 8:   pix<8>; transposed 8 -> 5: the generic kernel transposed; weight gradient tiled, P = 128"""
    check(Ci, Co, 2, 9, 13, nchw_in, nchw_out)


@gpu
@pytest.mark.parametrize("Ci,Co,nchw_in", [(3, 180, True), (4, 64, False), (7, 5, False), (7, 32, False)])
def test_generic_kernels(Ci, Co, nchw_in):
    """Output channel counts the pixel-per-thread switch does not hold: conv3x3_kernel, on (2, 9, 13).
      3 -> 180, NCHW in (SwinIR conv_first): generic forward; transposed 180 -> 3: pix<3>; weight gradient generic
                (180 * 27 = 4860 outputs > 2048: SwinIR conv_first's in f32 mode)
      4 -> 64 (DRUNet's f32 head): generic forward and generic transposed (4 outputs, 64 inputs: no lane shape);
                weight gradient generic (64 * 36 = 2304)
      7 -> 5:   generic forward and transposed; weight gradient tiled, P = 128
      7 -> 32:  pix<32>; transposed 32 -> 7: generic (7 outputs); weight gradient tiled at the largest count it takes
                (32 * 63 = 2016 outputs <= 2048, eight per thread) with P = 128: 32 + 63 floats per pixel are 48,640 bytes,
                inside the 48 KiB (P = 64 and 16 are test_pixel_per_thread_kernels' 16 -> 3 and 64 -> 3)"""
    check(Ci, Co, 2, 9, 13, nchw_in, False)


@gpu
@pytest.mark.parametrize("which", ["y", "res", "bias"])
def test_misaligned_operand_falls_back_to_the_pixel_kernel(which):
    """3 -> 32 with y, res or bias one float off the 16-byte grid: conv3x3_small_to_c32_kernel reads and writes them as
    float4, so the dispatcher takes conv3x3_pix_kernel<32> instead. Within 5e-6 of float64, and within 2e-6 of the aligned
    launch (the same products, summed in a different order)."""
    import _native as N
    B, H, W = 2, 5, 17
    c = make_case(3, 32, B, H, W)
    conv = whole_reference(c)[0]
    xd, wd = c["x"].cuda(), c["w"].cuda()
    res, bias = nhwc(c["res"]).cuda(), c["b"].cuda()
    y_al = torch.full_like(res, float("nan"))
    N.call("sei_conv3x3_fwd", xd.data_ptr(), wd.data_ptr(), bias.data_ptr(), res.data_ptr(), y_al.data_ptr(), B, H, W, 3, 32, 1, 0, 0)
    y = at_offset(torch.zeros(res.shape), 1) if which == "y" else torch.full_like(res, float("nan"))
    if which == "res":
        res = at_offset(res, 1)
    if which == "bias":
        bias = at_offset(bias, 1)
    assert sum(t.data_ptr() % 16 != 0 for t in (y, res, bias)) == 1
    N.call("sei_conv3x3_fwd", xd.data_ptr(), wd.data_ptr(), bias.data_ptr(), res.data_ptr(), y.data_ptr(), B, H, W, 3, 32, 1, 0, 0)
    torch.cuda.synchronize()
    ref = conv + c["res"].double()
    errs = relerr(canon(y, False), ref), relerr(canon(y_al, False), ref), relerr(y, y_al)
    print(f"3->32 with {which} off the grid: {errs[0]:.2e} of float64 (aligned {errs[1]:.2e}), {errs[2]:.2e} of the aligned launch")
    assert errs[0] < FWD_BAR and errs[1] < FWD_BAR and errs[2] < 2e-6


# kernel -> (Cin, Cout, (B, H, W), nchw_in, nchw_out, deviations of float32 F.conv2d on the CPU from float64: forward, data
# gradient, weight gradient, bias gradient)
SECOND_TRIPS = {
    "generic forward": (3, 180, (3, 48, 48), True, False, (1.71e-7, 3.16e-7, 1.04e-6, 6.77e-7)),
    "small_to_c32": (3, 32, (1, 1030, 1024), True, False, (1.96e-7, 3.41e-7, 5.52e-6, 3.89e-6)),
    "pix": (8, 3, (1, 1450, 1450), False, False, (3.25e-7, 1.73e-7, 3.677e-5, 3.618e-5)),
    "c32_to_small": (32, 3, (1, 524400, 1), False, True, (2.38e-7, 1.26e-7, 4.64e-6, 1.420e-5)),
    "tiled weight gradient": (3, 8, (1, 370, 370), False, False, (1.43e-7, 2.37e-7, 2.73e-6, 2.40e-6)),
    "generic weight gradient": (3, 180, (1, 370, 370), True, False, (2.17e-7, 2.31e-7, 6.804e-6, 7.933e-6)),
}


@gpu
@pytest.mark.parametrize("kernel", sorted(SECOND_TRIPS))
def test_second_trips_of_the_grid_stride_loops(kernel):
    """The smallest shapes that pass the grid caps of the dispatcher, so that a workgroup takes a second trip of its loop:
      generic forward          3 -> 180 on (3, 48, 48):    1,244,160 outputs > 4096 workgroups * 256
      small_to_c32             3 -> 32 on (1, 1030, 1024): 1,054,720 pixels > 16384 * 64 (four lanes per pixel)
      pix                      8 -> 3 on (1, 1450, 1450):  2,102,500 pixels > 8192 * 256
      c32_to_small             32 -> 3 on (1, 524400, 1):  one run per row, 524,400 runs > 65535 * 8
      tiled weight gradient    3 -> 8 on (1, 370, 370):    136,900 pixels > 1024 tiles of 128: tiles_per_block = 2
      generic weight gradient  3 -> 180 on (1, 370, 370):  136,900 pixels > 2048 * 64: pix_per_block = 128
    The forward and the data gradient are compared at a fixed random sample of 4096 pixels plus all four borders; the
    weight and bias gradients whole.
    Float32 F.conv2d on the CPU deviates from float64 by at most 3.4e-7 in the forward and the data gradient of these
    cases (SECOND_TRIPS has every figure): those bars stay at 5e-6. Its weight and bias gradients, sums over up to
    2.1 million pixels, deviate by more than a third of 2e-5 in three cases, whose bars are three times the deviation:
      pix:                     weight gradient 3.68e-5 -> bar 1.10e-4, bias gradient 3.62e-5 -> bar 1.09e-4
      c32_to_small:            bias gradient 1.42e-5 -> bar 4.26e-5 (weight gradient 4.6e-6: 2e-5 stays)
      generic weight gradient: weight gradient 6.80e-6 -> bar 2.04e-5, bias gradient 7.93e-6 -> bar 2.38e-5"""
    Ci, Co, (B, H, W), nchw_in, nchw_out, f32 = SECOND_TRIPS[kernel]
    bars = tuple(bar_for(b, d) for b, d in zip((FWD_BAR, FWD_BAR, WGRAD_BAR, WGRAD_BAR), f32))
    check(Ci, Co, B, H, W, nchw_in, nchw_out, sampled=True, bars=bars)


@gpu
def test_weights_beyond_the_staged_64_kib_are_refused():
    """sei_conv3x3_fwd stages its weights in at most 64 KiB of LDS: 64 -> 32 channels are 73,728 bytes. It returns
    SEI_ERR_TOO_LARGE before anything is launched and the output buffer keeps its contents."""
    import _native as N
    B, H, W = 1, 4, 5
    x, w = torch.randn((B, H, W, 64)).cuda(), torch.randn((32, 64, 3, 3)).cuda()
    y = torch.full((B, H, W, 32), -7.0, device="cuda")
    for transposed in (0, 1):
        with pytest.raises(N.NativeLibraryError, match="SEI_ERR_TOO_LARGE"):
            N.call("sei_conv3x3_fwd", x.data_ptr(), w.data_ptr(), None, None, y.data_ptr(), B, H, W, 64, 32, 0, 0, transposed)
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())
