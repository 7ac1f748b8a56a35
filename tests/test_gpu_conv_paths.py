"""GPU: every conv kernel on every loader / epilogue path and every plane shape it admits, against the float64 restatement of
tests/conv_ref.py.

Part one forces each shape id of conv_kernels.h through mcvd_op_conv2d on the paths the model runs -- raw input, the GroupNorm affine,
affine + SiLU (the kernels' fast exp / reciprocal), a virtual concat with the seam on a chunk boundary and a residual scaled by
0.70710678, a ragged last chunk (40 channels in 48), a padded cout tile (Cout 5 and 40), 8 x 8 planes with an odd batch (two images per
workgroup or pixel tile), the K splits at their smallest Cin -- on Gaussian data, and the affine + SiLU and concat rows on constant,
dominant-channel and cancelling data for one id per arithmetic.  Part two runs affine + SiLU + residual on the planes that are not
square (8x16, 16x32, 32x16, 24x16, 8x32; 4x8 for the 1x1 GEMMs with B = 4, 5, 6: four images per pixel tile) for every id the dispatcher
launches, the planes the admission rule refuses (the next id of the fallback list must run) and the GroupNorm partials on 8x16 and 16x32.

Every case asserts the id that ran (conv_ref.expected_id: the fallback lists, tests/wino_rule.admits and a restatement of the two 1x1
predicates, never the library's answer), that two launches agree bit for bit, and err = max |y - y64| / mag with
mag = max (conv(|xin|, |w|) + |bias| + |res|) * scale.

Gates (none invented here):
  * fp32 products (ids 0 .. 9): err < 2e-6, the absolute gate of test_conv_bf16x3_is_fp32_accurate and test_conv1x1_split_operand_accuracy.
    A plain fp32 torch evaluation of the same expressions on the CPU stays below 1.8e-7.
  * three bf16 pieces (10, 11, 15): err < 2e-6 and err <= max(1.5 err_f, 2e-7) with err_f the fp32-MFMA id of the family on the same
    data (4, 8, 5): the rule of those two tests.  Both ids share the fast SiLU, so its error cancels out of the ratio.
  * 16 / 17 / 20 are bit-equal to 10 / 11 / 18 (with persist_grid 0, 1 and 7); 18 / 19 lie within 2e-6 max(|y|, 1) of id 10
    (tests/test_gpu_ksplit_deep.py, tests/test_gpu_wino3p.py).
  * two fp16 pieces (12, 13, 26; 14) on Gaussian data: <= max(2 err_f, 1e-6) and < 6e-6 for Winograd with test_conv_f16x2_accuracy's
    normaliser max |y64|; <= max(2 err_f, 1e-6) and < 4e-6 for id 14 with test_conv1x1_split_operand_accuracy's normaliser (mag).
    On the structured kinds the figure is printed and recorded, NOTHING is asserted on it (the id that ran and bit-equal launches still
    are): the 2^-22 operand error does not average out there and no derived bound exists.  On `dominant` ids 12 and 14 return
    non-finite values: a channel of 1e4 standard deviations times the activation scale leaves the fp16 range (|d| < 1023,
    conv_wino2h.cpp H2_ACT_SCALE), which is what the model's range guard reports (test_f16x2_overflow_is_reported_...); recorded as such.
  * one fp16 piece (24, 25, 27): per element, the derived bound of tests/f16x1_ref.py as
    test_forced_one_piece_kernel_meets_the_derived_bound applies it (conv_ref.f16x1_bound adds the epilogue's roundings of the residual).
  * GroupNorm partials: the count of tests/gn_ref.expected_np, nothing written behind the pairs, sum and M2 within 1e-4 of the largest
    value (tests/test_gpu_gn_partials.py).

measure() returns the figures, tools/conv_paths_accuracy.py prints them, profiles/conv_paths_accuracy.txt holds the worst per id and path.

Measured on the MI355X (366 cases, no kernel had to change and no plane had to be refused): every admitted launch meets its gate.  The
worst line is id 15 on 4x8 planes with B = 5 (four images per pixel tile, a ragged last tile): err 1.5e-7, 0.77 of max(1.5 err_f, 2e-7),
i.e. of the 2e-7 floor; id 15 lies between 0.49 and 0.77 of that gate on every path (id 5, its err_f, is as accurate as it), ids 10 / 11
below 0.58, and all three below 0.16 of 2e-6.  The fp32 ids: the 256- and
128-pixel direct tiles (0, 1) reach 9.9e-7 (0.50 of 2e-6) on `dominant` behind affine + SiLU and 6.2e-7 on 16x32 planes, three to eight
times the split-K tiles 2 / 3 and the Winograd and DMA kernels (4, 8: <= 8.4e-8 on Gaussian data; 5, 6, 9: <= 2.1e-7).  Two-piece ids on
Gaussian data: <= 2.6e-7 (0.26 of the 1e-6 floor); one-piece ids: <= 0.11 of the derived bound; 18 / 19 within 0.16 of their distance gate
to id 10; 16 / 17 / 20 bit-equal to 10 / 11 / 18 at every plane and grid.  GroupNorm partials on 8x16 and 16x32: <= 0.011 of the 1e-4 gate.
"""
import pytest
import torch

from tests import conv_ref as CR
from tests import gn_ref

pytestmark = pytest.mark.gpu

TABLE = CR.kernel_table()
FP32_IDS = (0, 1, 2, 3, 4, 5, 6, 8, 9)
THREE = (10, 11, 15)
TWO_WINO, TWO_1X1 = (12, 13, 26), (14,)
ONE = (24, 25, 27)
FP32_BASE = {10: 4, 11: 8, 15: 5, 12: 4, 13: 8, 26: 8, 14: 5}       # the fp32-MFMA id of the same family (26: CF_WINO has no 4-way split)
BIT_EQUAL = {16: 10, 17: 11, 20: 18}
NEAR_10 = (18, 19)
KS1 = ("DMA1", "SPLIT1")


def _ks(kid):
    return 1 if TABLE[kid][0] in KS1 else 3


# ------------------------------------------------------------------------------------------------ part one: loader and epilogue paths
IDS3 = (0, 1, 2, 3, 4, 8, 10, 11, 12, 13, 24)
IDS1 = (5, 6, 9, 14, 15)
KINDS_IDS = (0, 4, 5, 10, 15, 12, 14)
KSPLIT_MIN = ((8, 64), (11, 64), (13, 64), (25, 64), (18, 128), (19, 256), (26, 192), (27, 192))


def _rows(kid, kind="gauss"):
    """{path: [cases]} of the table of paths, for one id."""
    c = CR.case
    if _ks(kid) == 3:
        return {
            "raw": [c(kid, 3, 2, 64, 0, 40, 16, coef=False, act=0, kind=kind)],
            "affine": [c(kid, 3, 2, 64, 0, 40, 16, act=0, kind=kind)],
            "silu": [c(kid, 3, 2, 64, 0, 40, 16, kind=kind)],
            "concat": [c(kid, 3, 3, 48, 16, 96, 16, res=True, kind=kind)],
            "ragged": [c(kid, 3, 2, 40, 0, 64, 16, kind=kind)],
            "cout5": [c(kid, 3, 2, 64, 0, 5, 16, kind=kind)],
            "g8": [c(kid, 3, 3, 48, 16, 96, 8, res=True, kind=kind)],
        }
    return {
        "raw": [c(kid, 1, 2, 96, 0, 96, 16, coef=False, act=0, kind=kind)],
        "affine": [c(kid, 1, 2, 96, 0, 96, 16, act=0, kind=kind)],
        "silu": [c(kid, 1, 2, 96, 0, 96, 16, kind=kind)],
        "concat": [c(kid, 1, 2, 64, 32, 96, 16, res=True, kind=kind)],
        "ragged": [c(kid, 1, 3, 72, 0, 64, 16, res=True, kind=kind)],          # Cin no multiple of 16: the direct tile takes the launch
        "cout40": [c(kid, 1, 2, 96, 0, 40, 16, kind=kind)],
        "g8": [c(kid, 1, 3, 288, 0, 288, 8, res=True, kind=kind), c(kid, 1, 5, 288, 0, 288, 8, res=True, kind=kind)],
    }


def _part_one():
    out = []
    for kid in IDS3 + IDS1:
        for path, cases in _rows(kid).items():
            for cs in cases:
                if CR.expected_id(cs, TABLE) == kid or (path == "ragged" and _ks(kid) == 1):       # where the id serves the path
                    out.append((path, cs))
    for kid in (0, 1, 2, 3):                                                                   # the direct tiles take any C0
        out.append(("concat5+5", CR.case(kid, 3, 2, 5, 5, 40, 16, res=True)))
    for kid, cin in KSPLIT_MIN:
        out += [("ksplit", CR.case(kid, 3, 3, cin, 0, 40, 8, res=True)), ("ksplit", CR.case(kid, 3, 2, cin, 0, 40, 16, res=True))]
    for kid in KINDS_IDS:
        for kind in ("const", "dominant", "cancel"):
            rows = _rows(kid, kind)
            out += [("silu", rows["silu"][0]), ("concat", rows["concat"][0])]
    return out


PART_ONE = _part_one()

# ------------------------------------------------------------------------------------------------ part two: planes
PLANES = [(8, 16), (16, 32), (32, 16), (24, 16), (8, 32)]
STATS_IDS = (0, 4, 5, 10, 12, 15, 11)
# planes the rule (or a 1x1 predicate) refuses: (forced id, plane, the id that must run)
REFUSED = [(4, (12, 16), "direct"), (10, (12, 16), "direct"), (12, (12, 16), "direct"), (16, (12, 16), "direct"), (24, (12, 16), "direct"),
           (11, (12, 16), "direct"), (10, (16, 8), "direct"), (16, (8, 8), 10), (17, (8, 8), 11), (20, (8, 8), 11), (9, (4, 8), "direct"),
           (9, (24, 16), "direct")]          # id 9: 256-pixel tiles take whole multiples of 256 pixels, or up to four whole images


def _part_two():
    out = []
    for kid in CR.dispatcher_ids():
        ks, cin = _ks(kid), CR.min_cin(kid, TABLE)
        for plane in PLANES:
            for pgrid in ((0, 1, 7) if kid in BIT_EQUAL else (0,)):
                out.append(("plane", CR.case(kid, ks, 3, cin, 0, 40, plane, res=True, pgrid=pgrid)))
        if ks == 1:
            out += [("plane", CR.case(kid, 1, B, cin, 0, 40, (4, 8), res=True)) for B in (4, 5, 6)]
    for kid, plane, _ in REFUSED:
        cs = CR.case(kid, _ks(kid), 3, CR.min_cin(kid, TABLE), 0, 40, plane, res=True)
        if ("plane", cs) not in out:
            out.append(("refused", cs))
    for kid in STATS_IDS:
        out += [("stats", CR.case(kid, _ks(kid), 3, CR.min_cin(kid, TABLE), 0, 40, plane, res=True, stats=True)) for plane in ((8, 16), (16, 32))]
    return out


PART_TWO = _part_two()


@pytest.fixture(scope="module")
def ctx():
    from tests.hiputil import Ctx
    return Ctx()


# ------------------------------------------------------------------------------------------------ measure
_RUNS = {}


def _bit_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))       # (NaN == NaN where the bits agree)


def _run(ctx, c):
    """One forced launch, twice: (the id that ran, y on the CPU, repeatable, GroupNorm figures or None).  Kept per case: the fp32-MFMA and
    bit-equal partners of a case are launched once."""
    if c in _RUNS:
        return _RUNS[c]
    from mcvd_pytorch_amd import _lib
    t = CR.inputs(c)
    dev = lambda v: v.cuda().contiguous() if v is not None else None
    args = (dev(t["x0"]), dev(t["w"]), dev(t["bias"]))
    kw = dict(x1=dev(t["x1"]), coef=dev(t["coef"]), act=c.act, res=dev(t["res"]), scale=t["scale"])
    st = None
    try:
        ctx.opt("conv_shape", c.kid)
        ctx.opt("conv_cot", c.cot)
        ctx.opt("persist_grid", c.pgrid)
        if c.stats:
            y, part, np_, buf = ctx.conv2d_stats_full(*args, **kw)
            ran = _lib.lib.mcvd_last_conv_kernel()
            y2, part2, np2, _ = ctx.conv2d_stats_full(*args, **kw)
            same = _bit_equal(y, y2) and np_ == np2 and (np_ == 0 or _bit_equal(part, part2))
            used = c.B * c.Cout * np_ * 2
            st = dict(np=np_, written_finite=bool(torch.isfinite(buf[:used]).all()), rest_untouched=bool(torch.isnan(buf[used:]).all()))
            if np_:
                want_sum, want_m2 = gn_ref.tensor_moments(y)
                got_sum, got_m2 = gn_ref.fold_partials(part, c.H * c.W)
                st["sum_ratio"] = (got_sum - want_sum).abs().max().item() / (1e-4 * max(want_sum.abs().max().item(), 1.0))
                st["m2_ratio"] = (got_m2 - want_m2).abs().max().item() / (1e-4 * want_m2.abs().max().item())
        else:
            y = ctx.conv2d(*args, **kw)
            ran = _lib.lib.mcvd_last_conv_kernel()
            same = _bit_equal(y, ctx.conv2d(*args, **kw))
    finally:
        ctx.opt("conv_shape", -1)
        ctx.opt("conv_cot", 0)
        ctx.opt("persist_grid", 0)
    _RUNS[c] = (ran, y.cpu(), same, st)
    return _RUNS[c]


def _partner(c, kid):
    return c._replace(kid=kid, cot=0, pgrid=0, stats=False)


def measure(ctx, c):
    """Run one case; returns the figures and `gates`: [(name, value, limit, strict)] with value < limit (strict) or <= limit asserted by the
    test, and `recorded`: figures nothing is asserted on."""
    want = CR.expected_id(c, TABLE)
    ran, y, same, st = _run(ctx, c)
    y64, mag = CR.reference(c), CR.mag(c)
    diff = (y.double() - y64).abs()
    err = diff.max().item() / mag
    out = dict(ran=ran, want=want, repeatable=same, finite=bool(torch.isfinite(y).all()), err=err, mag=mag, gates=[], recorded=[], stats=st,
               assert_finite=True)
    gate_id = ran if want == "direct" else want              # the arithmetic that must have run decides the gate
    gates = out["gates"]

    def partner_err(kid, norm):
        p = _partner(c, kid)
        pran, py, _, _ = _run(ctx, p)
        assert pran == kid, f"the partner id {kid} of {CR.case_id(c)} did not run ({pran} did)"
        return (py.double() - y64).abs().max().item() / norm, py

    if gate_id in FP32_IDS:
        gates.append(("err", err, 2e-6, True))
    elif gate_id in THREE:
        err_f, _ = partner_err(FP32_BASE[gate_id], mag)
        out["err_f"] = err_f
        gates += [("err", err, 2e-6, True), ("err vs fp32-MFMA", err, max(1.5 * err_f, 2e-7), False)]
    elif gate_id in BIT_EQUAL:
        _, py = partner_err(BIT_EQUAL[gate_id], mag)
        gates.append(("differs from id %d" % BIT_EQUAL[gate_id], 0.0 if torch.equal(y, py) else (y - py).abs().max().item() + 1e-30, 0.0, False))
    elif gate_id in NEAR_10:
        _, py = partner_err(10, mag)
        gates.append(("|y - y10|", (y - py).abs().max().item(), 2e-6 * max(py.abs().max().item(), 1.0), False))
    elif gate_id in TWO_WINO or gate_id in TWO_1X1:
        norm = y64.abs().max().item() if gate_id in TWO_WINO else mag
        err_n = diff.max().item() / norm
        err_f, _ = partner_err(FP32_BASE[gate_id], norm)
        out["err_f"] = err_f
        cap = 6e-6 if gate_id in TWO_WINO else 4e-6
        if c.kind == "gauss":
            gates += [("err (own normaliser)", err_n, cap, True), ("err vs fp32-MFMA", err_n, max(2.0 * err_f, 1e-6), False)]
        else:
            out["recorded"] += [("err (own normaliser)", err_n), ("fp32-MFMA", err_f), ("finite", float(out["finite"]))]
            out["assert_finite"] = False      # `dominant`: 1e4 times the activation scale leaves the fp16 range (what the range guard reports)
    elif gate_id in ONE:
        gates.append(("|err| / bound", (diff / CR.f16x1_bound(c)).max().item(), 1.0, False))
    else:
        raise AssertionError(f"no gate for id {gate_id}")
    if st is not None:
        want_np = gn_ref.expected_np(ran, c.H, c.W, c.B)
        out["want_np"] = want_np
        if st["np"]:
            gates += [("folded sum", st["sum_ratio"], 1.0, False), ("folded M2", st["m2_ratio"], 1.0, False)]
    return out


def check(c, r):
    assert CR.ran_as_expected(r["ran"], r["want"]), f"kernel {r['ran']} ran, {r['want']} must"
    assert r["finite"] or not r["assert_finite"], "a value is not finite"
    assert r["repeatable"], "two launches differ"
    for name, value, limit, strict in r["gates"]:
        assert (value < limit) if strict else (value <= limit), f"{name}: {value:.3e}, gate {limit:.3e} (id {r['ran']}, {CR.case_id(c)})"
    st = r["stats"]
    if st is not None:
        assert st["np"] == r["want_np"], f"np {st['np']}, the launcher's rule gives {r['want_np']}"
        assert st["written_finite"], "a partial of the B * Cout * np pairs was not written (or is not finite)"
        assert st["rest_untouched"], "the kernel wrote behind its B * Cout * np pairs"


def _show(path, c, r):
    print(path, CR.case_id(c), {k: v for k, v in r.items() if k != "stats"}, r["stats"] or "")


@pytest.mark.parametrize("path,case", PART_ONE, ids=lambda v: v if isinstance(v, str) else CR.case_id(v))
def test_loader_and_epilogue_paths(ctx, path, case):
    r = measure(ctx, case)
    _show(path, case, r)
    check(case, r)


@pytest.mark.parametrize("path,case", PART_TWO, ids=lambda v: v if isinstance(v, str) else CR.case_id(v))
def test_planes_the_admission_rules_take_and_refuse(ctx, path, case):
    r = measure(ctx, case)
    _show(path, case, r)
    check(case, r)
    if path == "refused":
        forced_family = TABLE[case.kid][0]
        assert r["ran"] != case.kid and TABLE[r["ran"]][0] != forced_family, f"{forced_family} ran on a plane its rule refuses"
