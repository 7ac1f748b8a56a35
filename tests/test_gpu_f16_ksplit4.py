"""GPU: the 4-way K split of the two fp16 Winograd kernels -- shape ids 26 (wino2h_k4, two-piece operands, conv_wino2h.cpp) and 27
(wino1h_k4, one-piece operands, the same file with NP = 1) -- forced through the stand-alone conv.

blockIdx.y picks one of four parts of the 16-channel chunks, every part writes its raw partial result, launch_wino_ksplit_reduce sums
them in a fixed order: the split only reorders the fp32 accumulation, so each id is held to what its 2-way form is held to --
  * 27: per element, the bound tests/f16x1_ref.py derives for the one-piece arithmetic, against an fp64 convolution
    (tests/test_gpu_f16x1.py: test_forced_one_piece_kernel_meets_the_derived_bound);
  * 26: the assertion of tests/test_gpu_parity.py: test_conv_f16x2_accuracy -- worst-element error over the output scale within 2 x the
    fp32-MFMA Winograd kernel's (id 4) on the same data and below 6e-6.
The shapes are the smallest at which one mechanism can break (the K split exists at H * W <= 256 only); the last one is the refusal: 18
chunks do not divide by 4, and the launch must take the next id of the fallback list (13 / 25), not 26 / 27 and not silently something else.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import f16x1_ref as R

pytestmark = pytest.mark.gpu

MINCH_K4 = 3                     # conv_wino2h.cpp, both piece counts: chunks per part, at least (tests/test_f16_ksplit4_cpu.py checks the source)
SHAPES = [
    # (B, C0, C1, Cout, H, chunks divide by 4)
    (2, 16 * 4 * MINCH_K4, 0, 32, 8, True),     # G8, the shortest admissible parts, COT 1
    (3, 256, 0, 96, 8, True),                   # G8, odd batch: the last workgroup's second image is empty; COT 3
    (2, 160, 96, 64, 16, True),                 # concat whose seam falls inside a part (chunk 10 of 16); regions instead of G8; COT 2
    (3, 288, 0, 96, 8, False),                  # 18 chunks, not divisible by 4: refused, the 2-way form runs
]
MAGNITUDES = [(1.0, 1.0), (1e-3, 30.0), (40.0, 0.02)]


@pytest.fixture(scope="module")
def ctx():
    from tests.hiputil import Ctx
    return Ctx()


def _case(B, C0, C1, Cout, H, wscale, xscale):
    g = torch.Generator().manual_seed(31)
    Cin = C0 + C1
    x = torch.randn(B, Cin, H, H, generator=g) * xscale
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5 * wscale
    bias = 0.1 * torch.randn(Cout, generator=g) * wscale * xscale
    coef = torch.stack([(1 + 0.3 * torch.randn(B, Cin, generator=g)), 0.3 * xscale * torch.randn(B, Cin, generator=g)], -1).contiguous()
    return x, w, bias, coef


def _run(ctx, shape, x0, x1, w, bias, kw):
    from mcvd_pytorch_amd import _lib
    ctx.opt("conv_shape", shape)
    try:
        y = ctx.conv2d(x0, w, bias, x1=x1, **kw)
        return y, _lib.lib.mcvd_last_conv_kernel()
    finally:
        ctx.opt("conv_shape", -1)


@pytest.mark.parametrize("wscale,xscale", MAGNITUDES, ids=["unit", "small_w_big_x", "big_w_small_x"])
@pytest.mark.parametrize("B,C0,C1,Cout,H,divides", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", [26, 27], ids=["wino2h_k4", "wino1h_k4"])
def test_forced_four_way_split_meets_its_arithmetic_s_gate(ctx, shape, B, C0, C1, Cout, H, divides, wscale, xscale):
    x, w, bias, coef = _case(B, C0, C1, Cout, H, wscale, xscale)
    x0, x1 = (x[:, :C0].contiguous().cuda(), x[:, C0:].contiguous().cuda()) if C1 else (x.cuda(), None)
    wd, bd = w.cuda(), bias.cuda()
    want_id = shape if divides else {26: 13, 27: 25}[shape]
    for pro in (0, 1, 2):                                        # raw, affine, affine + SiLU
        kw = dict(coef=coef.cuda() if pro else None, act=1 if pro == 2 else 0)
        got, ran = _run(ctx, shape, x0, x1, wd, bd, kw)
        assert ran == want_id, f"forced {shape}, ran {ran}, expected {want_id}"
        again, _ = _run(ctx, shape, x0, x1, wd, bd, kw)
        three, _ = _run(ctx, 18, x0, x1, wd, bd, kw)             # the three-piece bf16 4-way split (its own fallback on the last shape)
        assert torch.isfinite(got).all()
        assert torch.equal(got, again), f"pro {pro}: two runs differ"
        assert not torch.equal(got, three), f"pro {pro}: bit-equal to the three-piece kernel's output: the fp16 pieces did not run"
        d = R.activate(x, coef if pro else None, pro == 2)
        y64 = F.conv2d(d, w.double(), bias.double(), padding=1)
        err = (got.cpu().double() - y64).abs()
        rel = err.max().item() / y64.abs().max().item()
        if shape == 27:
            _, bound = R.wino_f16x1(d, w)
            bound = bound + 2.0 ** -23 * bias.double().abs().reshape(1, -1, 1, 1)
            ratio = (err / bound).max().item()
            print(f"id 27 (ran {ran}) B{B} {C0}+{C1}->{Cout} @{H} w*{wscale} x*{xscale} pro {pro}: worst |err| / bound {ratio:.4f}, max|err| / max|y| {rel:.2e}")
            assert (err <= bound).all(), f"pro {pro}: |err| / bound = {ratio:.3f}"
            assert rel > 1e-5, "fp32-sized error: one fp16 piece did not run"
        else:
            f32, ran4 = _run(ctx, 4, x0, x1, wd, bd, kw)         # the fp32-MFMA Winograd kernel on the same data
            assert ran4 == 4
            rel4 = (f32.cpu().double() - y64).abs().max().item() / y64.abs().max().item()
            print(f"id 26 (ran {ran}) B{B} {C0}+{C1}->{Cout} @{H} w*{wscale} x*{xscale} pro {pro}: fp32-MFMA {rel4:.3e}  f16x2 k4 {rel:.3e}")
            assert rel <= max(2.0 * rel4, 1e-6), f"pro {pro}: f16x2 conv error {rel:.3e} vs fp32-MFMA {rel4:.3e}"
            assert rel < 6e-6, rel
