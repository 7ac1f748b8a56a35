"""GPU: the admission rule of the Winograd 3x3 families (conv_kernels.h: kWinoRules / wino_admits), one launch per row of the rule.

Each case forces an id through the stand-alone conv (affine + SiLU over a per-(sample, channel) random table, B = 2, Cout = 32) and asserts
  * the id that RAN (mcvd_last_conv_kernel): the forced one where the rule admits the launch, else the first id of its fallback list
    (conv_kernels.h) the rule admits, else a direct tile (0 .. 3);
  * the result against an fp64 convolution under the standing gate 1e-4 * scale + 2e-5 * max(scale, 1).  The one row that RUNS a one-piece
    fp16 id (27; a draft arithmetic of 11-bit operands, which the standing gate was never the contract of: measured 1.41e-3 against a gate
    of 3.8e-4, on the commit before this file as on this one) is held to what tests/test_gpu_wide_conv.py holds ids 25 / 27 to: the
    per-element bound tests/f16x1_ref.py derives for that arithmetic (+ 2^-23 |bias|), and an error that shows one piece did run.

The stand-alone conv hands id 4 no K split and sizes the partial-result scratch for the parts of the FORCED id, so a fallback to fewer parts
always finds room.  The expectations were read off the rule, not off a run; tests/test_wino_rule_cpu.py evaluates the same table with the
Python restatement of the rule (tests/wino_rule.py) and the fallback lists.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import f16x1_ref as R
from tests.test_gpu_wide_conv import _case, _run

pytestmark = pytest.mark.gpu

TILE = "tile"          # any direct tile kernel, ids 0 .. 3
ONE_PIECE = (24, 25, 27)
B, COUT = 2, 32

CASES = [
    # (forced, C0, C1, plane, runs)
    (10, 1040, 0, 8, TILE),     # a part above 1024 channels at 8 x 8; id 4 likewise
    (11, 1056, 0, 8, 11),       # 66 chunks, 528 channels per part
    (11, 1040, 0, 8, TILE),     # 65 chunks: odd
    (18, 2304, 0, 8, 18),
    (19, 2304, 0, 8, 19),       # 18 chunks per part
    (19, 192, 0, 8, 18),        # 12 chunks do not divide by 8
    (12, 2048, 0, 8, TILE),
    (13, 2048, 0, 8, 13),       # 1024 channels per part
    (25, 2304, 0, 8, TILE),     # the channel bound of a 2-way split
    (8, 48, 0, 8, 4),           # 3 chunks: odd
    (16, 1040, 0, 16, 10),      # the persistent kernel stays at 1024 channels
    (16, 48, 0, 16, 10),        # 3 chunks, the persistent stream needs 4
    (17, 96, 0, 16, 16),        # 3 chunks per half
    (17, 1056, 0, 16, 11),
    (20, 2304, 0, 16, TILE),    # no 4-way persistent launch above 1024 channels, no 2-way launch above 2048
    (26, 128, 0, 16, 13),       # parts of 2 chunks, the 4-way prologue needs 3
    (27, 192, 0, 16, 27),
    (10, 8, 16, 16, TILE),      # the concat seam inside a chunk
]


@pytest.fixture(scope="module")
def ctx():
    from tests.hiputil import Ctx
    return Ctx()


@pytest.mark.parametrize("forced,C0,C1,H,runs", CASES, ids=lambda v: str(v))
def test_forced_id_runs_what_the_rule_says(ctx, forced, C0, C1, H, runs):
    x, w, bias, coef = _case(B, C0, C1, COUT, H)
    x0, x1 = (x[:, :C0].contiguous().cuda(), x[:, C0:].contiguous().cuda()) if C1 else (x.cuda(), None)
    got, ran = _run(ctx, forced, x0, x1, w.cuda(), bias.cuda(), dict(coef=coef.cuda(), act=1))
    d = R.activate(x, coef, True)
    y64 = F.conv2d(d, w.double(), bias.double(), padding=1)
    scale = y64.abs().max().item()
    err = (got.cpu().double() - y64).abs()
    gate = 1e-4 * scale + 2e-5 * max(scale, 1.0)
    print(f"forced {forced} at {C0}+{C1} channels, {H} x {H}: ran {ran}, max-abs err {err.max().item():.3e}, gate {gate:.3e} (scale {scale:.3f})")
    assert (0 <= ran <= 3) if runs == TILE else ran == runs, f"forced {forced} at {C0}+{C1} channels, {H} x {H}: ran {ran}, the rule says {runs}"
    assert torch.isfinite(got).all()
    if runs in ONE_PIECE:
        bound = R.wino_f16x1(d, w)[1] + 2.0 ** -23 * bias.double().abs().reshape(1, -1, 1, 1)
        print(f"    one piece: worst |err| / bound {(err / bound).max().item():.4f}")
        assert (err <= bound).all(), f"|err| / bound = {(err / bound).max().item():.3f}"
        assert err.max().item() > 1e-5 * scale, "fp32-sized error: one fp16 piece did not run"
    else:
        assert err.max().item() <= gate, f"max-abs err {err.max().item():.3e} above the gate {gate:.3e}"
