"""The banded resampler and the circular blurs on the dispatch paths the U-Net's own shapes never reach: launches with
more than 64 KiB of dynamic LDS (a real DIV2K photograph through the dataset resize; --kernel files of 37 to 63 taps),
the resampler's halved output tile above 160 KiB, and images smaller than the blur kernel (a halo that wraps more than
once). Reference: float64 on the CPU; the bar is the 2e-6 (max-norm relative) of tests/test_physics_gpu.py.

Where the float32 CPU evaluation of the same operation (F.interpolate, blur_fft) deviates from the float64 one by more
than a third of that bar, the case's bar is three times that deviation (the margin of the scale-transform test, for a
different summation order). Float32 blur_fft deviates by 2.7e-7 to 5.3e-7 at these shapes: no blur case widens it.
Float32 F.interpolate deviates by 1.25e-6 at the DIV2K ratio and 7.3e-7 at the reduction by 8 with the halved tile:
those two cases are held to 3.74e-6 and 2.19e-6 (RESIZES).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import closed_form as cf
from oracle import torch_path as tp

pytestmark = pytest.mark.gpu
TOL = 2e-6
LDS_DEFAULT, LDS_CU = 64 * 1024, 160 * 1024


def relerr(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def resample_bands_and_lds(hi, wi, ho, wo):
    """((step, band) of the rows, (step, band) of the columns, dynamic LDS bytes of the launch) for the antialiased resize
    hi x wi -> ho x wo, from the bands resample_to_size builds and the library's own query."""
    import _native
    from physics import _bands
    _, _, nbv, sv = _bands.to_band(_bands.aa_bicubic_matrix_to_size(hi, ho))
    _, _, nbh, sh = _bands.to_band(_bands.aa_bicubic_matrix_to_size(wi, wo))
    return (sv, nbv), (sh, nbh), _native.lib().sei_resample_sepband_lds(hi, wi, ho, wo, nbv, sv, nbh, sh)


# (input, output size, (step, band) of both axes, LDS bytes of the 16 x 32 tile, whether the launch keeps that tile, the
# deviation of float32 F.interpolate on the CPU from float64 on this test's input)
RESIZES = {
    "div2k-ratio": ((1, 2, 175, 361), (33, 68), (6, 22), 4 * (112 * 208 + 112 * 32), True, 1.247e-6),      # 105 KiB
    "under-the-limit": ((1, 1, 130, 270), (17, 35), (8, 31), 4 * (130 * 270 + 130 * 32), True, 5.93e-7),   # 153 KiB
    "halved-tile": ((1, 1, 260, 530), (33, 67), (8, 32), 4 * (152 * 280 + 152 * 32), False, 7.31e-7),      # 185 KiB
    "control": ((2, 3, 96, 130), (48, 65), None, None, True, 1.70e-7),
}


def bar_for(f32_deviation):
    """TOL, or three times the float32 CPU evaluation's own deviation where that exceeds a third of TOL."""
    return 3 * f32_deviation if f32_deviation > TOL / 3 else TOL


@pytest.mark.parametrize("case", sorted(RESIZES))
def test_antialiased_resize_at_the_ratios_of_real_photographs(case):
    """resample_to_size(antialias=True) (the GroundTruthDataset resize: sei_resample_sepband) against float64
    F.interpolate(bicubic, antialias=True, align_corners=False), at the smallest shapes that keep the ratios of a
    1356 x 2040 DIV2K image resized to 256 x 385 (step 6, band 22: 105 KiB of dynamic LDS) and of reductions by 8
    (153 KiB: just under a CU's 160 KiB; 185 KiB with the 16 x 32 output tile: the tile is halved, the call serves it),
    three ragged tiles per axis, beside a control below 64 KiB. Which regime a case sits in is asserted through
    sei_resample_sepband_lds. Float32 F.interpolate deviates from float64 by 1.25e-6, 5.9e-7, 7.3e-7 and 1.7e-7 in that
    order: the bars are 3.74e-6, 2e-6, 2.19e-6 and 2e-6."""
    from physics._ops import resample_to_size
    shape, (ho, wo), band, full_tile_lds, keeps_tile, f32_deviation = RESIZES[case]
    bv, bh, lds = resample_bands_and_lds(shape[2], shape[3], ho, wo)
    if band is None:
        assert 0 < lds <= LDS_DEFAULT
    else:
        assert bv == band and bh == band
        assert LDS_DEFAULT < lds <= LDS_CU
        assert (lds == full_tile_lds) if keeps_tile else (full_tile_lds > LDS_CU)
    gen = torch.Generator().manual_seed(31)
    x = torch.rand(shape, generator=gen)
    ref = F.interpolate(x.double(), size=(ho, wo), mode="bicubic", antialias=True, align_corners=False)
    y = resample_to_size(x.cuda(), ho, wo, antialias=True)
    torch.cuda.synchronize()
    err = relerr(y, ref)
    print(f"{case}: lds {lds}, resize rel err {err:.2e}, bar {bar_for(f32_deviation):.2e}")
    assert err < bar_for(f32_deviation)


def rank1_kernel(kv, kh, seed):
    gen = torch.Generator().manual_seed(seed)
    tv = torch.rand(kv, generator=gen, dtype=torch.float64) + 0.05
    th = torch.rand(kh, generator=gen, dtype=torch.float64) + 0.05
    return torch.outer(tv / tv.sum(), th / th.sum())


# (kv, kh) -> whether a 64 x 64 tile with that halo takes more than 64 KiB: 4 * (128 + (63 + kv) (63 + kh) + (63 + kv) 64)
BIG_TAPS = {(37, 37): True, (63, 63): True, (63, 1): False, (62, 40): True}


@pytest.mark.parametrize("shape", [(1, 2, 64, 64), (1, 2, 70, 130)])
@pytest.mark.parametrize("taps", sorted(BIG_TAPS))
def test_separable_blur_with_many_taps(taps, shape):
    """BlurV2 through sei_blur_sep_circ with rank-1 kernels of 37 to 63 taps (what a --kernel file may carry; the table
    kernels stop at 19): 64 x 64 tiles whose halo takes 65 to 94 KiB of dynamic LDS, and 63 x 1 taps just under 64 KiB, on
    one whole tile and on ragged ones. A, A_adjoint and the autograd backward against float64 blur_fft and the direct
    circular correlation; <Ax, z> = <x, A^T z>. Float32 blur_fft deviates from float64 by 2.7e-7 to 5.3e-7 here."""
    import _native
    import physics
    kv, kh = taps
    k = rank1_kernel(kv, kh, seed=kv * 100 + kh)
    lds = _native.lib().sei_blur_sep_circ_lds(kv, kh, shape[2], shape[3])
    assert (LDS_DEFAULT < lds <= LDS_CU) if BIG_TAPS[taps] else (0 < lds <= LDS_DEFAULT)
    op = physics.BlurV2(kernel=k[None, None])
    assert op._op.separable
    gen = torch.Generator().manual_seed(17)
    x, z = torch.rand(shape, generator=gen), torch.rand(shape, generator=gen)
    ref = tp.blur_fft(x.double(), k)
    ref_adj = cf.blur_adjoint_direct(z.numpy(), k.numpy())
    xd = x.cuda().requires_grad_(True)
    y = op.A(xd)
    (gx,) = torch.autograd.grad(y, xd, z.cuda())
    adj = op.A_adjoint(z.cuda())
    torch.cuda.synchronize()
    errs = relerr(y, ref), relerr(adj, ref_adj), relerr(gx, ref_adj)
    print(f"taps {taps} on {shape}: lds {lds}, A {errs[0]:.2e}, A_adjoint {errs[1]:.2e}, backward {errs[2]:.2e}")
    assert max(errs) < TOL
    lhs = (y.detach().double() * z.cuda().double()).sum()
    rhs = (x.cuda().double() * adj.double()).sum()
    assert abs(lhs - rhs) / abs(lhs) < 1e-6


def folded_fft_blur(x, k):
    """blur_fft's route for a kernel that may be larger than the image: the PSF rolled to the origin and folded onto the
    H x W torus, then rfft2 * rfft2, irfft2, in float64."""
    H, W = x.shape[-2:]
    kv, kh = k.shape
    psf = torch.zeros((H, W), dtype=torch.float64)
    for a in range(kv):
        for b in range(kh):
            psf[(a - kv // 2) % H, (b - kh // 2) % W] += k[a, b]
    return torch.fft.irfft2(torch.fft.rfft2(x.double()) * torch.fft.rfft2(psf), s=(H, W))


@pytest.mark.parametrize("kind,shape", [("Gaussian_R3", (1, 1, 5, 7)), ("Gaussian_R3", (2, 1, 1, 3)), ("dense4x6", (1, 1, 3, 2))])
def test_blur_of_images_smaller_than_the_kernel(kind, shape):
    """The 19-tap Gaussian on 5 x 7 and 1 x 3 images (separable kernel) and a dense 4 x 6 kernel on a 3 x 2 image: the
    halo of the single tile wraps round the image more than once. A and A_adjoint against the float64 direct circular
    sums (oracle/closed_form.py) and against the FFT route with the PSF folded onto the image's torus (blur_fft itself
    cannot hold a PSF larger than the image)."""
    import physics
    if kind == "dense4x6":
        k = torch.rand((4, 6), generator=torch.Generator().manual_seed(6), dtype=torch.float64)
        k /= k.sum()
    else:
        k = tp.blur_kernel(kind)
    op = physics.BlurV2(kernel=k[None, None])
    assert op._op.separable == (kind != "dense4x6")
    gen = torch.Generator().manual_seed(23)
    x, z = torch.rand(shape, generator=gen), torch.rand(shape, generator=gen)
    y, adj = op.A(x.cuda()), op.A_adjoint(z.cuda())
    torch.cuda.synchronize()
    ref = cf.blur_direct(x.numpy(), k.numpy())
    assert relerr(folded_fft_blur(x, k), ref) < 1e-13          # the two float64 references agree
    assert relerr(y, ref) < TOL
    assert relerr(adj, cf.blur_adjoint_direct(z.numpy(), k.numpy())) < TOL
    lhs = (y.double() * z.cuda().double()).sum()
    rhs = (x.cuda().double() * adj.double()).sum()
    assert abs(lhs - rhs) / abs(lhs) < 1e-6


def test_a_64_tap_kernel_is_refused_and_nothing_is_written():
    """One tap above the limit: sei_blur_sep_circ returns SEI_ERR_TOO_LARGE (NativeLibraryError through the binding)
    before anything is launched -- the output buffer keeps its contents -- and the LDS query says 0."""
    import _native as N
    import physics
    k = rank1_kernel(64, 3, seed=64)
    op = physics.BlurV2(kernel=k[None, None])
    assert op._op.separable
    x = torch.rand((1, 2, 64, 64), generator=torch.Generator().manual_seed(3)).cuda()
    with pytest.raises(N.NativeLibraryError, match="SEI_ERR_TOO_LARGE"):
        op.A(x)
    with pytest.raises(N.NativeLibraryError, match="SEI_ERR_TOO_LARGE"):
        op.A_adjoint(x)
    tv, th = op._op._taps(x.device)
    y = torch.full_like(x, -7.0)
    for kv, kh, a, b in ((64, 3, tv, th), (3, 64, th, tv)):
        with pytest.raises(N.NativeLibraryError, match="SEI_ERR_TOO_LARGE"):
            N.call("sei_blur_sep_circ", x.data_ptr(), y.data_ptr(), a.data_ptr(), b.data_ptr(), kv, kh, 2, 64, 64, 0)
        assert N.lib().sei_blur_sep_circ_lds(kv, kh, 64, 64) == 0
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())
