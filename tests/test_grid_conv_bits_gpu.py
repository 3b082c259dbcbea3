"""GPU: the implicit-GEMM body that the DRUNet and the diffusion U-Net convolutions share (csrc/grid_conv.h).

(a) Every entry point on that body writes the bits recorded in tests/golden/g20_grid_conv_bits.json: the SHA-256 of each
    output buffer, whole, border and guard rows included. The inputs are seeded on the CPU, so they are the same bytes
    everywhere. The fixture was recorded on an MI355X at the commit before the two kernels were given one body, with

        python tests/test_grid_conv_bits_gpu.py --record

    which uses only entry points that commit has. The extents 2 x 5 x 7 give 126 grid rows: no multiple of 16, 32 or 64,
    so the clamped rows and the row tail run; 1 x 48 x 52 with 64 -> 512 channels gives 2700 rows and 43 x 8 = 344 waves,
    the 64-row default tile.
(b) sei_adm_conv with a zero bias and no residual and sei_drunet_conv3x3 with epilogue 1 on a zero trunk give float32
    outputs that are torch.equal: the two families are one body (acc + 0 and 0 + acc are both acc)."""
import functools
import hashlib
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                  # run as a script: the import paths that conftest.py sets for pytest
    for _p in (os.path.join(ROOT, "scale-equivariant-imaging_amd"), ROOT):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import pytest
import torch
from torch.nn import functional as F

import _native as N
from test_pnp_baseline_gpu import bf16_values, empty_grid, pack, to_grid, trunk_grid

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(ROOT, "tests", "golden", "g20_grid_conv_bits.json")
SMALL, BIG = (2, 5, 7), (1, 48, 52)
BF16, F32 = torch.bfloat16, torch.float32


@functools.lru_cache(maxsize=None)
def operands(Cin, Cout, ext, k=3):
    """(the input grid with its guard rows, the guard, the packed weights) of a k x k convolution, made once."""
    B, H, W = ext
    x = bf16_values((B, Cin, H, W), Cin + H)
    w = bf16_values((Cout, Cin, k, k), Cout + W, scale=math.sqrt(1.0 / (k * k * Cin)))
    xg, guard = to_grid(x)
    return xg, guard, pack(w)


def addend(Cout, ext, seed):
    B, H, W = ext
    return trunk_grid(bf16_values((B, Cout, H, W), seed))


def dr_conv(Cin, Cout, ext, epilogue, skip=False, pb=None, zero_trunk=False):
    B, H, W = ext
    xg, guard, wt = operands(Cin, Cout, ext)
    yg, _ = empty_grid(B, Cout, H, W, BF16)
    name, tail = ("sei_drunet_conv3x3", ()) if pb is None else ("sei_drunet_conv3x3_ex", (pb,))
    if epilogue == 0:
        N.call(name, xg[guard:].data_ptr(), wt.data_ptr(), Cin, Cout, B, H, W, 0, None, None, None, yg[guard:].data_ptr(), *tail)
        return {"y16": yg}
    tg, _ = empty_grid(B, Cout, H, W, F32)
    tin = torch.zeros_like(tg) if zero_trunk else addend(Cout, ext, 3)
    tsk = addend(Cout, ext, 4) if skip else None
    N.call(name, xg[guard:].data_ptr(), wt.data_ptr(), Cin, Cout, B, H, W, 1, tin.data_ptr(),
           None if tsk is None else tsk.data_ptr(), tg.data_ptr(), yg[guard:].data_ptr(), *tail)
    return {"t32": tg, "y16": yg}


def dr_masked(C, ext):
    B, H, W = ext
    xg, guard, wt = operands(C, C, ext)
    mask, _ = to_grid(bf16_values((B, C, H, W), 5))                    # about half of it above zero
    yg, _ = empty_grid(B, C, H, W, BF16)
    N.call("sei_drunet_conv3x3_masked", xg[guard:].data_ptr(), wt.data_ptr(), C, C, B, H, W, mask[guard:].data_ptr(),
           yg[guard:].data_ptr())
    return {"y16": yg}


def dr_down(Clo, Chi, ext):
    B, h, w = ext
    xg, guard = to_grid(bf16_values((B, Clo, 2 * h, 2 * w), Clo + h))
    wt = pack(bf16_values((Chi, Clo, 2, 2), 5, scale=math.sqrt(1.0 / (4 * Clo))))
    yg, g2 = empty_grid(B, Chi, h, w, BF16)
    tg, _ = empty_grid(B, Chi, h, w, F32)
    N.call("sei_drunet_down", xg[guard:].data_ptr(), wt.data_ptr(), Clo, Chi, B, h, w, tg.data_ptr(), yg[g2:].data_ptr())
    return {"t32": tg, "y16": yg}


def dr_up(Chi, Clo, ext):
    B, h, w = ext
    zg, g2 = to_grid(bf16_values((B, Chi, h, w), Chi + w))
    wu = bf16_values((Chi, Clo, 2, 2), 6, scale=math.sqrt(1.0 / Chi))
    wt = wu.permute(2, 3, 1, 0).reshape(4 * Clo, Chi).to(BF16).contiguous().cuda()
    yg, guard = empty_grid(B, Clo, 2 * h, 2 * w, BF16)
    tg, _ = empty_grid(B, Clo, 2 * h, 2 * w, F32)
    N.call("sei_drunet_up", zg[g2:].data_ptr(), wt.data_ptr(), Chi, Clo, B, h, w, tg.data_ptr(), yg[guard:].data_ptr())
    return {"t32": tg, "y16": yg}


def dr_head(ext, C=64):
    B, H, W = ext
    x = bf16_values((B, 3, H, W), 21, signed=False).float().cuda()
    wt = pack(F.pad(bf16_values((C, 4, 3, 3), 22, scale=math.sqrt(1.0 / 36)), (0, 0, 0, 0, 0, 28)))
    yg, guard = empty_grid(B, C, H, W, BF16)
    tg, _ = empty_grid(B, C, H, W, F32)
    work = torch.full((N.lib().sei_drunet_work_bytes(B, H, W),), 0x7F, dtype=torch.uint8, device="cuda")
    N.call("sei_drunet_head", x.data_ptr(), 0.05, wt.data_ptr(), C, B, H, W, tg.data_ptr(), yg[guard:].data_ptr(),
           work.data_ptr())
    return {"t32": tg, "y16": yg, "work": work}


def dr_tail(ext, C=64):
    B, H, W = ext
    zg, guard = to_grid(bf16_values((B, C, H, W), 23))
    wt = pack(F.pad(bf16_values((3, C, 3, 3), 24, scale=math.sqrt(1.0 / (9 * C))), (0, 0, 0, 0, 0, 0, 0, 13)))
    out = torch.full((B, 3, H, W), 9.0, device="cuda")
    N.call("sei_drunet_tail", zg[guard:].data_ptr(), wt.data_ptr(), C, B, H, W, out.data_ptr())
    return {"image": out}


def adm_conv(Cin, Cout, taps, ext, res=False, out32=True, out16=False, zero_bias=False):
    B, H, W = ext
    xg, guard, wt = operands(Cin, Cout, ext, 3 if taps == 9 else 1)
    bias = torch.zeros(Cout, device="cuda") if zero_bias else bf16_values((Cout,), 7, scale=0.5).float().cuda()
    rg = addend(Cout, ext, 3) if res else None
    out = {}
    if out32:
        out["t32"] = empty_grid(B, Cout, H, W, F32)[0]
    if out16:
        out["y16"] = empty_grid(B, Cout, H, W, BF16)[0]
    N.call("sei_adm_conv", xg[guard:].data_ptr(), wt.data_ptr(), bias.data_ptr(), Cin, Cout, taps, B, H, W,
           None if rg is None else rg.data_ptr(), out["t32"].data_ptr() if out32 else None,
           out["y16"][guard:].data_ptr() if out16 else None)
    return out


def adm_pack(ext):
    B, H, W = ext
    rows, guard = B * (H + 2) * (W + 2), W + 3
    g = torch.full((rows + 2 * guard, 32), 3.0, dtype=BF16, device="cuda")
    x = bf16_values((B, 3, H, W), 21).float().cuda()
    N.call("sei_adm_pack_image", x.data_ptr(), g[guard:].data_ptr(), B, H, W)
    return {"grid": g}


def adm_tail(ext, C=128):
    B, H, W = ext
    zg, guard = to_grid(bf16_values((B, C, H, W), 24))
    wt = pack(F.pad(bf16_values((3, C, 3, 3), 25, scale=math.sqrt(1.0 / (9 * C))), (0, 0, 0, 0, 0, 0, 0, 13)))
    bias = F.pad(bf16_values((3,), 26, scale=0.5), (0, 13)).float().cuda()
    out = torch.full((B, 3, H, W), 9.0, device="cuda")
    N.call("sei_adm_tail", zg[guard:].data_ptr(), wt.data_ptr(), bias.data_ptr(), C, B, H, W, out.data_ptr())
    return {"image": out}


CASES = {
    "drunet_conv3x3 relu 64->128": lambda: dr_conv(64, 128, SMALL, 0),
    "drunet_conv3x3 residual 64->128": lambda: dr_conv(64, 128, SMALL, 1),
    "drunet_conv3x3 residual+skip 64->128": lambda: dr_conv(64, 128, SMALL, 1, skip=True),
    "drunet_conv3x3_ex pb=1 C=64": lambda: dr_conv(64, 64, SMALL, 1, skip=True, pb=1),
    "drunet_conv3x3_ex pb=2 C=64": lambda: dr_conv(64, 64, SMALL, 1, skip=True, pb=2),
    "drunet_conv3x3_ex pb=4 C=64": lambda: dr_conv(64, 64, SMALL, 1, skip=True, pb=4),
    "drunet_conv3x3_masked C=64": lambda: dr_masked(64, SMALL),
    "drunet_down 64->128": lambda: dr_down(64, 128, SMALL),
    "drunet_up 128->64": lambda: dr_up(128, 64, SMALL),
    "drunet_head": lambda: dr_head(SMALL),
    "drunet_tail": lambda: dr_tail(SMALL),
    "drunet_conv3x3 residual 64->512 64-row tile": lambda: dr_conv(64, 512, BIG, 1),
    "adm_conv 3x3 384->128 bias": lambda: adm_conv(384, 128, 9, SMALL),
    "adm_conv 3x3 384->128 residual, both outputs": lambda: adm_conv(384, 128, 9, SMALL, res=True, out16=True),
    "adm_conv 3x3 384->128 bf16 only": lambda: adm_conv(384, 128, 9, SMALL, out32=False, out16=True),
    "adm_conv 3x3 128->128 bias": lambda: adm_conv(128, 128, 9, SMALL),
    "adm_conv 3x3 128->128 residual, both outputs": lambda: adm_conv(128, 128, 9, SMALL, res=True, out16=True),
    "adm_conv 3x3 128->128 bf16 only": lambda: adm_conv(128, 128, 9, SMALL, out32=False, out16=True),
    "adm_conv 1x1 384->128": lambda: adm_conv(384, 128, 1, SMALL, out16=True),
    "adm_pack_image": lambda: adm_pack(SMALL),
    "adm_tail": lambda: adm_tail(SMALL),
    "adm_conv 3x3 64->512 64-row tile": lambda: adm_conv(64, 512, 9, BIG, res=True, out16=True),
}


def digests(buffers):
    torch.cuda.synchronize()
    return {k: hashlib.sha256(v.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest() for k, v in buffers.items()}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_the_cases(recorded):
    assert sorted(recorded["digests"]) == sorted(CASES)


@pytest.mark.parametrize("case", list(CASES))
def test_same_bits_as_recorded(recorded, case):
    got = digests(CASES[case]())
    assert got == recorded["digests"][case], f"{case}: the fixture was recorded with {recorded['hipcc']!r}"


SAME_BODY = [(64, 128, SMALL), (128, 128, SMALL), (64, 128, BIG), (128, 128, BIG), (64, 512, BIG)]


@pytest.mark.parametrize("Cin,Cout,ext", SAME_BODY)
def test_both_families_give_the_same_bits(Cin, Cout, ext):
    adm = adm_conv(Cin, Cout, 9, ext, zero_bias=True)["t32"]
    dr = dr_conv(Cin, Cout, ext, 1, zero_trunk=True)["t32"]
    assert float(adm.abs().max()) > 0.0 and torch.equal(adm, dr)


def record():
    import subprocess
    for Cin, Cout, ext in SAME_BODY:
        test_both_families_give_the_same_bits(Cin, Cout, ext)
        print(f"same body {Cin}->{Cout} {ext}: equal", flush=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    version = subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout.splitlines()[0]
    out = {"hipcc": version, "device": torch.cuda.get_device_name(0), "digests": {k: digests(fn()) for k, fn in CASES.items()}}
    again = {k: digests(fn()) for k, fn in CASES.items()}
    assert again == out["digests"], "the bits differ between two runs"
    with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(CASES)} cases with {version!r}", flush=True)


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        sys.exit("usage: python tests/test_grid_conv_bits_gpu.py --record [OUT.json]")
    record()
