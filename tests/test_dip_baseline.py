"""The Deep Image Prior baseline without a GPU: the decoder's stage extents, the parameter bucket against torch's own modules,
the model factory, and the host-side argument checks of the sei_dip_* entry points."""
import pytest
import torch

from models.dip import ConvDecoderParams, DeepImagePrior, decoder_sizes


def test_decoder_sizes():
    assert [h for h, _ in decoder_sizes((256, 256))] == [26, 41, 64, 102, 162, 256]
    assert decoder_sizes((256, 256))[3] == (102, 102)
    assert decoder_sizes((40, 56)) == [(19, 20), (22, 25), (26, 30), (30, 37), (35, 46), (40, 56)]
    assert decoder_sizes((12, 20)) == [(16, 17), (15, 18), (14, 18), (14, 19), (13, 20), (12, 20)]      # extents may shrink
    assert decoder_sizes((9, 13), in_size=(4, 4), layers=3) == [(6, 8), (9, 13)]
    assert decoder_sizes((1, 5), in_size=(4, 4), layers=2) == [(1, 5)]


def test_parameter_bucket_is_torch_s_initialisation_in_module_order():
    torch.manual_seed(3)
    params = ConvDecoderParams((3, 40, 56))
    assert params.numel == params.flat.numel() == 7 * (9216 + 32 + 64) + 99 == 65283
    assert params.flat.dtype == torch.float32
    # the same modules, written out here, under the same seed
    torch.manual_seed(3)
    ch, mods = 32, []
    for hw in decoder_sizes((40, 56)):
        mods += [torch.nn.Upsample(size=hw, mode="nearest"), torch.nn.Conv2d(ch, ch, 3, 1, padding=1), torch.nn.ReLU(),
                 torch.nn.BatchNorm2d(ch)]
    mods += [torch.nn.Conv2d(ch, ch, 3, 1, padding=1), torch.nn.ReLU(), torch.nn.BatchNorm2d(ch), torch.nn.Conv2d(ch, 3, 1)]
    seq = torch.nn.Sequential(*mods)
    stages, head = params.views(params.flat)
    convs = [m for m in seq if isinstance(m, torch.nn.Conv2d)]
    norms = [m for m in seq if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(stages) == 7 == len(norms) and len(convs) == 8
    for st, conv, bn in zip(stages, convs, norms):
        assert torch.equal(st["w"], conv.weight) and torch.equal(st["b"], conv.bias)
        assert torch.equal(st["gamma"], bn.weight) and torch.equal(st["beta"], bn.bias)
        assert st["w"].shape == (32, 32, 3, 3)
    assert torch.equal(head["w"], convs[-1].weight) and torch.equal(head["b"], convs[-1].bias)
    assert head["w"].shape == (3, 32, 1, 1)
    assert torch.equal(params.flat, torch.cat([p.detach().reshape(-1) for p in seq.parameters()]))
    # stage l reads in_hw(l) and writes out_hw(l); the last conv stage keeps the size
    assert params.in_hw(0) == (16, 16) and params.out_hw(0) == (19, 20)
    assert params.in_hw(6) == params.out_hw(6) == params.out_hw(5) == (40, 56)


def _args(*flags, **extra):
    """The common parser's arguments plus test.py's own --dip_iterations (default None)."""
    from settings import DefaultArgParser
    args = DefaultArgParser().parse_args(list(flags))
    args.dip_iterations = extra.get("dip_iterations")
    return args


class StubPhysics:
    task = "deblurring"


def test_get_model_builds_the_dip_baseline():
    from models import get_model

    def built(*flags, **extra):
        return get_model(_args("--model_kind", "DeepImagePrior", *flags, **extra), physics=StubPhysics(), device="cpu")

    model = built("--task", "deblurring", "--kernel", "Gaussian_R2")
    dip = model.get_backbone()
    assert isinstance(dip, DeepImagePrior) and len(model.get_weights()) == 0 and list(model.parameters()) == []
    model.load_weights({})
    assert dip.iterations == 4000 and dip.lr == 5e-3 and dip.channels == 32 and dip.in_size == [16, 16] and dip.graph
    assert dip.sr_factor is None
    assert built("--task", "deblurring", "--kernel", "Box_R2").get_backbone().iterations == 1000
    sr = built("--task", "sr", "--sr_factor", "2").get_backbone()
    assert sr.iterations == 1000 and sr.sr_factor == 2
    assert built("--task", "deblurring", "--kernel", "Gaussian_R2", dip_iterations=7).get_backbone().iterations == 7
    assert built("--task", "invert_a_tomography_like_filter", dip_iterations=9).get_backbone().iterations == 9
    with pytest.raises(ValueError, match="dip_iterations"):
        built("--task", "invert_a_tomography_like_filter")
    with pytest.raises(NotImplementedError, match="operator"):
        get_model(_args("--model_kind", "DeepImagePrior", "--task", "sr", "--sr_factor", "2"), physics=None, device="cpu")
    with pytest.raises(ValueError, match="Unknown model kind"):
        get_model(_args("--model_kind", "dip", "--task", "sr", "--sr_factor", "2"), physics=StubPhysics(), device="cpu")


def test_the_baseline_refuses_cpu_tensors():
    import _native
    with pytest.raises(_native.NativeLibraryError):
        DeepImagePrior(StubPhysics(), iterations=2)(torch.rand(1, 3, 16, 16))


def test_entry_points_check_their_arguments_on_the_host():
    import _native
    sig, L = _native.SIGNATURES, _native.lib()
    assert [len(sig[n]) for n in ("sei_dip_stage_fwd", "sei_dip_head_fwd", "sei_dip_head_bwd", "sei_dip_stage_bwd_bn",
                                  "sei_dip_stage_bwd_data", "sei_dip_stage_bwd_weight", "sei_dip_adam")] == \
        [16, 10, 13, 10, 9, 12, 7]
    assert len(_native.SIZE_QUERIES["sei_dip_work_floats"]) == 4
    BAD = 10001
    p = [4096 * (i + 1) for i in range(8)]                        # fake, disjoint, 16-byte aligned

    def each_null(call, nptr, optional=()):
        """`call(pointers)` with every required pointer NULL in turn, and all of them NULL."""
        assert call([None] * nptr) == BAD
        for i in range(nptr):
            if i not in optional:
                assert call([None if j == i else p[j] for j in range(nptr)]) == BAD, i

    extents = [(0, 8, 8, 8), (8, 0, 8, 8), (8, 8, 0, 8), (8, 8, 8, -1)]
    each_null(lambda a: L.sei_dip_stage_fwd(*a, 8, 8, 8, 8, 32, 1e-5, None if a[0] is None else p[7] + 4096, None), 8,
              optional=(1,))
    assert L.sei_dip_stage_fwd(*p[:8], 8, 8, 8, 8, 32, 1e-5, None, None) == BAD                   # work
    each_null(lambda a: L.sei_dip_head_fwd(*a, 8, 8, 32, 3, None), 5)
    each_null(lambda a: L.sei_dip_head_bwd(*a[:7], 8, 8, 32, 3, a[7], None), 8)
    each_null(lambda a: L.sei_dip_stage_bwd_bn(a[0], a[1], a[2], a[3], None if a[3] is None else a[3] + 128, 8, 8, 32, a[4],
                                               None), 5)
    assert L.sei_dip_stage_bwd_bn(p[0], p[1], p[2], p[3], None, 8, 8, 32, p[4], None) == BAD
    assert L.sei_dip_stage_bwd_bn(p[0], p[1], p[2], p[3], p[5], 8, 8, 32, p[4], None) == BAD      # g_beta not behind g_gamma
    each_null(lambda a: L.sei_dip_stage_bwd_data(*a, 8, 8, 8, 8, 32, None), 3)
    each_null(lambda a: L.sei_dip_stage_bwd_weight(*a[:5], 8, 8, 8, 8, 32, a[5], None), 6, optional=(2,))
    each_null(lambda a: L.sei_dip_adam(a[0], a[1], a[2], a[3], 64, a[4], None), 5)
    assert L.sei_dip_adam(p[0], p[1], p[2], p[3], 0, p[4], None) == BAD
    for hi, wi, ho, wo in extents:
        assert L.sei_dip_stage_fwd(*p[:8], hi, wi, ho, wo, 32, 1e-5, p[7] + 4096, None) == BAD
        assert L.sei_dip_stage_bwd_data(*p[:3], hi, wi, ho, wo, 32, None) == BAD
        assert L.sei_dip_stage_bwd_weight(*p[:5], hi, wi, ho, wo, 32, p[5], None) == BAD
    for h, w in ((0, 8), (8, 0), (-1, 8)):
        assert L.sei_dip_head_fwd(*p[:5], h, w, 32, 3, None) == BAD
        assert L.sei_dip_head_bwd(*p[:7], h, w, 32, 3, p[7], None) == BAD
        assert L.sei_dip_stage_bwd_bn(p[0], p[1], p[2], p[3], p[3] + 128, h, w, 32, p[4], None) == BAD
        assert L.sei_dip_work_floats(h, w, 32, 3) == 0
    for c in (31, 33, 64, 0):                                       # built for 32 channels
        assert L.sei_dip_stage_fwd(*p[:8], 8, 8, 8, 8, c, 1e-5, p[7] + 4096, None) == BAD
        assert L.sei_dip_head_fwd(*p[:5], 8, 8, c, 3, None) == BAD
        assert L.sei_dip_head_bwd(*p[:7], 8, 8, c, 3, p[7], None) == BAD
        assert L.sei_dip_stage_bwd_bn(p[0], p[1], p[2], p[3], p[3] + 128, 8, 8, c, p[4], None) == BAD
        assert L.sei_dip_stage_bwd_data(*p[:3], 8, 8, 8, 8, c, None) == BAD
        assert L.sei_dip_stage_bwd_weight(*p[:5], 8, 8, 8, 8, c, p[5], None) == BAD
        assert L.sei_dip_work_floats(8, 8, c, 3) == 0
    for cout in (0, 9, -1):
        assert L.sei_dip_head_fwd(*p[:5], 8, 8, 32, cout, None) == BAD
        assert L.sei_dip_head_bwd(*p[:7], 8, 8, 32, cout, p[7], None) == BAD
        assert L.sei_dip_work_floats(8, 8, 32, cout) == 0
    assert L.sei_dip_stage_fwd(p[0] + 4, *p[1:8], 8, 8, 8, 8, 32, 1e-5, p[7] + 4096, None) == BAD   # activations: 16 bytes
    assert L.sei_dip_stage_fwd(*p[:8], 8, 8, 8, 8, 32, 0.0, p[7] + 4096, None) == BAD               # eps
    assert L.sei_dip_stage_fwd(*p[:8], 8, 8, 8, 16385, 32, 1e-5, p[7] + 4096, None) == 10002
    # the workspace: one partial block of the weight gradient (9216 + 32 floats) per 8 x 32 tile, at most 512 of them
    assert L.sei_dip_work_floats(1, 5, 32, 3) == 9248
    assert L.sei_dip_work_floats(40, 56, 32, 3) == 5 * 2 * 9248
    assert L.sei_dip_work_floats(256, 256, 32, 3) == 256 * 9248
    assert L.sei_dip_work_floats(1024, 1024, 32, 3) == 512 * 9248
