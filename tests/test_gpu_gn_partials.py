"""GPU: every conv kernel's GroupNorm partials, and both reducers, against the float64 restatement of tests/gn_ref.py.

Part one forces each shape id of conv_kernels.h through mcvd_op_conv2d and looks at what the epilogue (or the K split's reduce pass) left in
ConvArgs::stats: the id that ran, the number of partials, that exactly B * Cout * np pairs were written and nothing behind them, that two
launches agree bit for bit, that the partials fold (in float64) to the per-channel sum and M2 of the kernel's own output, and that
gn_finalize makes the float64 coefficients of that output from them.  Part two feeds gn_finalize partials computed in float64 and gn_coef
tensors, at the group shapes and loop edges of the two kernels, and compares with the float64 coefficients.

Gates (none invented here): sum and M2 within 1e-4 of the largest value (test_gpu_ksplit_deep.py); coefficients within
rtol 2e-5 + atol 2e-6 * max(1, |mean * rstd * par0|) (test_conv_epilogue_group_norm_statistics, the atol scaled as
test_wino2h_epilogue_statistics_with_a_large_mean scales it); the `offset` kind within that test's rtol 5e-5 + atol 2e-6 * |offset|.

Ids that write no partials are listed in DOES_NOT_EMIT; tests/test_gn_ref_cpu.py checks that every id of the header is in CASES with an
emitting case or in that set.  Id 2 is there with 3: both are the split-K direct tile (conv_mfma_dispatch_shape: SPLIT = true), whose
launcher never sets a partial count.  ksplit_reduce_gn_kernel (the reduce pass that also writes the table) is launched by the model only
(ConvArgs::gno is not an argument of mcvd_op_conv2d); behind the K-split ids this file checks the plain reduce pass.

gn_coef, data kind `outlier_first` (a unit Gaussian group whose first element is 1e3 / 3e4): a numpy emulation of the kernel as it was --
one pilot, the group's first element, var = E[(x-p)^2] - E[x-p]^2 -- put rstd off by 1.8e-4 (4 x 32x32, 1e3) to 1.2e-3 (3 x 64x64, 3e4).
Measured on the MI355X with that kernel, on this file's data: rstd off by 2.5e-4 (4 x 32x32, 1e3: 4.8 x the gate), 3.5e-4 (4 x 32x32, 3e4:
0.73 x, the gate's absolute part is large beside A = 0.07 there), 1.2e-3 (3 x 64x64, 1e3: 31 x) and 6.9e-4 (3 x 64x64, 3e4: 2.5 x); with the
outlier at element 1777 all four at 1e-7.  The kernel now merges per-float4 means pairwise: 1e-7 wherever the outlier sits
(profiles/gn_partials_accuracy.txt, profiles/gn_coef_time.txt).

Worst coefficient error per family, as a fraction of the gate (tools/gn_partials_accuracy.py; in brackets the multiple of a plain float32
two-pass on the CPU): direct tile 0.075 (24 x, id 0, offset -300), fp32 Winograd 0.031 (3.4 x, id 4, 8x8), bf16x3 Winograd 0.111 (25 x,
id 10, corner), persistent 0.113 (28 x, id 16, corner), f16x2 Winograd 0.106 (29 x, id 12, offset -300), f16x1 Winograd 0.105 (27 x, id 24,
offset -300), K split 0.032 (6 x, id 26 over a concat), all-DMA 1x1 0.050 (12 x, id 5, offset -300), split-operand 1x1 0.081 (17 x,
id 15, corner).  The pilot-shifted epilogues lose a decimal digit to a spike or a mean of 300 standard deviations at the pilot; a
tenth of the gate.
"""
import pytest
import torch

from oracle import unet_ref
from tests import gn_ref

pytestmark = pytest.mark.gpu

EPS = 1e-5
KS1 = ("DMA1", "SPLIT1")

# ids that never write partials, and why
DOES_NOT_EMIT = {
    2: "split-K direct tile (SPLIT = true): four waves hold partial channel sums, no wave has a final value to take moments of",
    3: "split-K direct tile with the double-buffered weight chunk: as 2",
    22: "3x3 as a 1x1 GEMM over shifted taps: launched by the model with ConvArgs::stats unset, not served by the dispatcher",
    23: "3x3 as a 1x1 GEMM over an im2col copy: as 22",
}


def _c(kid, B, C0, C1, Cout, H, kind="gauss", cot=0, pgrid=0):
    return (kid, B, C0, C1, Cout, H, kind, cot, pgrid)


def _case_id(c):
    kid, B, C0, C1, Cout, H, kind, cot, pgrid = c
    return f"{gn_ref.KERNELS[kid][0].lower()}{kid}_B{B}_c{C0}+{C1}_o{Cout}_H{H}_{kind}" + (f"_cot{cot}" if cot else "") + (f"_g{pgrid}" if pgrid else "")


CASES = []
# ---- unsplit Winograd: np = 2 with a padded cout tile (40 of 64) and the co < Cout predicate; two 8x8 images per workgroup, odd batch, np = 1;
# np = 8 with Cout = 5
for kid in (4, 10, 12, 24):
    CASES += [_c(kid, 3, 64, 0, 40, 16), _c(kid, 3, 48, 16, 96, 8), _c(kid, 1, 64, 0, 5, 32)]
# ---- persistent: the same planes at the family's minimum chunk count (WP_MINCH = 4 chunks per item: 64 / 128 / 256 channels for 16 / 17 / 20),
# with 1 and 7 workgroups so that a workgroup's run of items crosses samples
for pgrid in (1, 7):
    CASES += [_c(16, 3, 64, 0, 40, 16, pgrid=pgrid), _c(16, 1, 64, 0, 5, 32, pgrid=pgrid),
              _c(17, 3, 128, 0, 40, 16, pgrid=pgrid), _c(20, 3, 256, 0, 40, 16, pgrid=pgrid)]
CASES += [_c(17, 1, 128, 0, 5, 32, pgrid=7), _c(20, 1, 256, 0, 5, 32, pgrid=7)]          # planes above 16x16 behind a split: np = 0
# ---- K split: 8x8 with an odd batch and 16x16, each at the smallest Cin the id's usable() admits
#   8 / 11 / 13 / 25: an even number of 16-channel chunks, at least 4                      -> 64
#   18: chunks a multiple of 4, at least 8 -> 128;   19: a multiple of 8, at least 16       -> 256
#   26 / 27: a multiple of 4 with H2_MINCH_K4 = 3 chunks per part (both piece counts)   -> 192
for kid, cin in ((8, 64), (11, 64), (13, 64), (25, 64), (18, 128), (19, 256), (26, 192), (27, 192)):
    CASES += [_c(kid, 3, cin, 0, 40, 8), _c(kid, 2, cin, 0, 40, 16)]
CASES += [_c(18, 2, 160, 96, 96, 16), _c(26, 2, 160, 96, 96, 16)]      # a concat, the seam (chunk 10 of 16) inside part 2
CASES += [_c(kid, 1, 64, 0, 40, 32) for kid in (8, 11, 13, 25)]        # 32x32, one id per family: np = 0
# ---- all-DMA 1x1: a ragged last pixel tile (5 images of 64 pixels, 128 / 256 per tile), np = 2; one 256-pixel tile exactly
for kid in (5, 6, 9):
    CASES += [_c(kid, 5, 288, 0, 288, 8), _c(kid, 1, 96, 0, 40, 16)]
# ---- split-operand 1x1, cout tiles 1 and 3 (2 where the padded Cout has two 32-channel tiles): two images per tile and np = 1; fewer than
# eight pixel tiles (the block map of such launches); 32x32; at least eight pixel tiles
for kid in (14, 15):
    CASES += [_c(kid, 3, 288, 0, 288, 8, cot=1), _c(kid, 3, 288, 0, 288, 8, cot=3), _c(kid, 1, 96, 0, 40, 16, cot=1), _c(kid, 1, 96, 0, 40, 16, cot=2),
              _c(kid, 2, 96, 0, 96, 32, cot=1), _c(kid, 2, 96, 0, 96, 32, cot=3), _c(kid, 2, 96, 0, 96, 64, cot=1), _c(kid, 2, 96, 0, 96, 64, cot=3)]
# ---- direct tile: a tile emits from the first plane that fills it with one image (256 pixels for id 0, 128 for id 1; 16x16 is the smallest
# square plane with either) and not below; the split-K tiles never
CASES += [_c(0, 3, 10, 0, 96, 16), _c(0, 3, 10, 0, 96, 8), _c(1, 3, 64, 0, 40, 16), _c(1, 3, 64, 0, 40, 8), _c(1, 1, 32, 0, 40, 32),
          _c(2, 3, 64, 0, 40, 16), _c(2, 2, 64, 0, 40, 8), _c(3, 3, 64, 0, 40, 16)]
# ---- data kinds, one shape per family
for kid, shp in ((4, (2, 64, 0, 40, 16)), (10, (2, 64, 0, 40, 16)), (12, (2, 64, 0, 40, 16)), (24, (2, 64, 0, 40, 16)), (16, (2, 64, 0, 40, 16)),
                 (11, (2, 64, 0, 40, 16)), (5, (2, 96, 0, 96, 16)), (15, (2, 96, 0, 96, 16)), (0, (2, 64, 0, 40, 16))):
    CASES += [_c(kid, *shp, kind="const"), _c(kid, *shp, kind="corner")]
for kid, shp in ((10, (3, 64, 0, 96, 16)), (15, (3, 96, 0, 96, 16)), (5, (3, 96, 0, 96, 16)), (0, (3, 64, 0, 96, 16)), (24, (3, 64, 0, 96, 16)),
                 (12, (3, 64, 0, 96, 16))):
    CASES += [_c(kid, *shp, kind="offset+40"), _c(kid, *shp, kind="offset-300")]


@pytest.fixture(scope="module")
def ctx():
    from tests.hiputil import Ctx
    return Ctx()


def _inputs(case):
    kid, B, C0, C1, Cout, H, kind, cot, pgrid = case
    ks = 1 if gn_ref.KERNELS[kid][0] in KS1 else 3
    g = torch.Generator().manual_seed(1000 + kid)
    Cin = C0 + C1
    x0 = torch.randn(B, C0, H, H, generator=g)
    x1 = torch.randn(B, C1, H, H, generator=g) if C1 else None
    w = torch.randn(Cout, Cin, ks, ks, generator=g) / (Cin * ks * ks) ** 0.5
    bias = 0.5 + 0.1 * torch.randn(Cout, generator=g)
    coef = torch.stack([1 + 0.3 * torch.randn(B, Cin, generator=g), 0.3 * torch.randn(B, Cin, generator=g)], dim=-1) if ks == 3 else None
    res, scale = torch.randn(B, Cout, H, H, generator=g), 0.70710678
    if kind.startswith("offset"):
        bias, res, scale = float(kind[6:]) + torch.randn(Cout, generator=g), None, 1.0
    elif kind == "const":                    # y is exactly one multiple of 1/8 per group: zero weights, nothing added or scaled, every sum exact
        G = unet_ref.gn_groups(Cout)
        w, res, scale = torch.zeros_like(w), None, 1.0
        bias = (torch.randint(-16, 17, (G,), generator=g) / 8.0).repeat_interleave(Cout // G)
    elif kind == "corner":                   # the epilogues' pilot is a partial's first value: make the first value of the plane a spike
        res[:, :, 0, 0] = 1e3
    emb = 0.3 * torch.randn(B, 2 * Cout + 11, generator=g)
    return ks, x0, x1, w, bias, coef, res, scale, emb


def _ratio(got, want, rtol, atol):
    """max |got - want| / (rtol |want| + atol): 1.0 is the gate."""
    return ((got.double() - want).abs() / (rtol * want.abs() + atol)).max().item()


def measure(ctx, case):
    """Run one case; returns the figures the test asserts on (tools/gn_partials_accuracy.py prints them)."""
    from mcvd_pytorch_amd import _lib
    kid, B, C0, C1, Cout, H, kind, cot, pgrid = case
    ks, x0, x1, w, bias, coef, res, scale, emb = _inputs(case)
    dev = lambda t: t.cuda().contiguous() if t is not None else None
    args = (dev(x0), dev(w), dev(bias))
    kw = dict(x1=dev(x1), coef=dev(coef), act=1 if coef is not None else 0, res=dev(res), scale=scale)
    HW = H * H
    try:
        ctx.opt("conv_shape", kid)
        ctx.opt("conv_cot", cot)
        ctx.opt("persist_grid", pgrid)
        y, st, np_, buf = ctx.conv2d_stats_full(*args, **kw)
        ran = _lib.lib.mcvd_last_conv_kernel()
        y2, st2, np2, _ = ctx.conv2d_stats_full(*args, **kw)
    finally:
        ctx.opt("conv_shape", -1)
        ctx.opt("conv_cot", 0)
        ctx.opt("persist_grid", 0)
    out = dict(ran=ran, np=np_, want_np=gn_ref.expected_np(kid, H, H, B), y=y)
    used = B * Cout * np_ * 2
    out["written_finite"] = bool(torch.isfinite(buf[:used]).all())
    out["rest_untouched"] = bool(torch.isnan(buf[used:]).all())
    out["repeatable"] = torch.equal(y, y2) and np_ == np2 and (np_ == 0 or torch.equal(st, st2))
    if np_ == 0:
        return out
    want_sum, want_m2 = gn_ref.tensor_moments(y)
    got_sum, got_m2 = gn_ref.fold_partials(st, HW)
    out["sum_ratio"] = (got_sum - want_sum).abs().max().item() / (1e-4 * max(want_sum.abs().max().item(), 1.0))
    out["m2_max"] = want_m2.abs().max().item()
    out["m2_err"] = (got_m2 - want_m2).abs().max().item()
    out["partial_m2_max"] = st[..., 1].abs().max().item()
    G = unet_ref.gn_groups(Cout)
    mean, var = gn_ref.group_moments([("tensor", y)], HW, G)
    off = float(kind[6:]) if kind.startswith("offset") else None
    embd = emb.cuda()
    out["coef_ratio"] = 0.0
    for mode in (0, 1):
        p = dict(p0=emb, emb_off=7) if mode else {}
        want = gn_ref.coefficients(mean, var, EPS, mode, Cout, **p)
        got = ctx.gn_finalize(st, np_, G, EPS, mode, HW, **(dict(p0=embd, emb_stride=emb.shape[1], emb_off=7) if mode else {})).cpu()
        if off is None:
            rtol, atol = 2e-5, gn_ref.gate_atol(mean, var, EPS, mode, Cout, **p)
        else:
            rtol, atol = 5e-5, 2e-6 * abs(off)
        out[f"coef_ratio{mode}"] = _ratio(got, want, rtol, atol)
        out["coef_ratio"] = max(out["coef_ratio"], out[f"coef_ratio{mode}"])
        if mode == 0:
            out["A"] = got[..., 0]
            # the reference's own fp32 error, for the record: a plain two-pass mean / variance of the same y in float32 on the CPU
            yg = y.cpu().view(B, G, -1)
            m32 = yg.mean(-1, keepdim=True)
            v32 = ((yg - m32) ** 2).mean(-1, keepdim=True)
            a32 = (1.0 / torch.sqrt(v32 + EPS)).expand(B, G, Cout // G).reshape(B, Cout)
            b32 = (-m32 / torch.sqrt(v32 + EPS)).expand(B, G, Cout // G).reshape(B, Cout)
            out["ref32_ratio"] = _ratio(torch.stack([a32, b32], -1), want, rtol, atol)
    return out


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_producer_partials(ctx, case):
    kid, B, C0, C1, Cout, H, kind, cot, pgrid = case
    r = measure(ctx, case)
    print({k: v for k, v in r.items() if k not in ("y", "A")})
    assert r["ran"] == kid, f"kernel {r['ran']} ran, {kid} was asked for"
    assert r["np"] == r["want_np"], f"np {r['np']}, the launcher's rule gives {r['want_np']}"
    assert r["written_finite"], "a partial of the B * Cout * np pairs was not written (or is not finite)"
    assert r["rest_untouched"], "the kernel wrote behind its B * Cout * np pairs"
    assert r["repeatable"], "two launches differ"
    if r["np"] == 0:
        return
    assert r["sum_ratio"] <= 1.0, f"folded sum off by {r['sum_ratio']:.3g} x the gate (1e-4 of the largest sum)"
    if kind == "const":
        assert r["partial_m2_max"] == 0.0, f"a constant plane has M2 {r['partial_m2_max']:.3e}"
        assert r["m2_err"] == 0.0 and r["m2_max"] == 0.0
        want_a = 1.0 / EPS ** 0.5
        assert ((r["A"].double() - want_a).abs() <= 1e-6 * want_a).all()
    else:
        assert r["m2_err"] <= 1e-4 * r["m2_max"], f"folded M2 off by {r['m2_err']:.3e}, largest M2 {r['m2_max']:.3e}"
    assert r["coef_ratio0"] <= 1.0, f"mode 0 coefficients at {r['coef_ratio0']:.3g} x the gate"
    assert r["coef_ratio1"] <= 1.0, f"mode 1 coefficients at {r['coef_ratio1']:.3g} x the gate"


# ------------------------------------------------------------------------------------------------ the reducers alone
# (name, B, C0, C1, HW, groups, np0, np1)
REDUCER_SHAPES = [
    ("c2304_g32", 3, 2304, 0, 64, 32, 2, 1),          # 72 channels per group: the cl >= 64 tail loop of gn_finalize_kernel
    ("c1188+1116_seam", 3, 1188, 1116, 64, 32, 32, 1),   # the seam in the middle of group 16 (channels 1152 .. 1223), np0 = 32, np1 = 1
    ("gs4_np256", 3, 16, 0, 1024, 4, 256, 1),         # P = 1024 partials per group: the loop beyond GF_KEEP * 64 = 512
    ("gs1", 3, 8, 0, 64, 8, 2, 1),
]
# groups of n4 float4s at the edges of gn_coef_kernel's loops: HW = 16 (the smallest plane a conv writes), fewer float4s than threads, and both
# sides of `i + 256 < n4`
COEF_EDGE_SHAPES = [
    ("hw16", 3, 8, 0, 16, 2, 1, 1),                   # n4 = 16
    ("n4_64", 3, 8, 0, 64, 2, 1, 1),                  # n4 = 64
    ("n4_257", 2, 514, 0, 4, 2, 1, 1),                # 257 channels of one float4
    ("n4_511", 2, 14, 0, 292, 2, 1, 1),               # 7 x 73
    ("n4_512", 2, 16, 0, 256, 2, 1, 1),
    ("n4_513", 2, 54, 0, 76, 2, 1, 1),                # 27 x 19
]


def _data(shape, kind, seed=77):
    name, B, C0, C1, HW, G, np0, np1 = shape
    g = torch.Generator().manual_seed(seed)
    C = C0 + C1
    x = torch.randn(B, C, HW, generator=g) * (0.5 + torch.rand(B, C, 1, generator=g)) + 0.4 * torch.randn(B, C, 1, generator=g)
    if kind.startswith("offset"):
        x = x + float(kind[6:])
    elif kind == "const":
        x = (torch.randint(-16, 17, (B, G, 1, 1), generator=g) / 8.0).expand(B, G, C // G, HW).reshape(B, C, HW).clone()
    emb = 0.3 * torch.randn(B, 2 * C + 13, generator=g)
    wgt, bia = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    return x.contiguous(), emb, wgt, bia


def _mode_args(mode, emb, wgt, bia):
    """(reference keywords, kernel keywords)"""
    if mode == 1:
        return dict(p0=emb, emb_off=9), dict(p0=emb.cuda(), emb_stride=emb.shape[1], emb_off=9)
    if mode == 2:
        return dict(p0=wgt, p1=bia), dict(p0=wgt.cuda(), p1=bia.cuda())
    return {}, {}


def _check_coef(got, x, shape, mode, rk, what):
    name, B, C0, C1, HW, G, np0, np1 = shape
    C = C0 + C1
    mean, var = gn_ref.group_moments([("tensor", x)], HW, G)
    want = gn_ref.coefficients(mean, var, EPS, mode, C, **rk)
    r = _ratio(got.cpu(), want, 2e-5, gn_ref.gate_atol(mean, var, EPS, mode, C, **rk))
    print(f"{what} {name} mode {mode}: {r:.3g} x the gate")
    assert r <= 1.0, f"{what} {name} mode {mode}: coefficients at {r:.3g} x the gate"
    return want


def _partials64(x, np_):
    """[B, C, HW] -> [B, C, np, 2] (sum, M2 about the partial's own mean) of consecutive runs, computed in float64 and rounded to float32."""
    B, C, HW = x.shape
    xp = x.double().view(B, C, np_, HW // np_)
    return torch.stack([xp.sum(-1), ((xp - xp.mean(-1, keepdim=True)) ** 2).sum(-1)], -1).float()


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", REDUCER_SHAPES, ids=lambda s: s[0])
def test_gn_finalize_against_the_float64_fold(ctx, shape, mode):
    name, B, C0, C1, HW, G, np0, np1 = shape
    x, emb, wgt, bia = _data(shape, "gauss")
    rk, kk = _mode_args(mode, emb, wgt, bia)
    st0 = _partials64(x[:, :C0], np0)
    st1 = _partials64(x[:, C0:], np1) if C1 else None
    # the reference folds the SAME rounded partials: what is compared is the kernel's fold, not the rounding of its input
    mean, var = gn_ref.group_moments([("partials", st0)] + ([("partials", st1)] if C1 else []), HW, G)
    want = gn_ref.coefficients(mean, var, EPS, mode, C0 + C1, **rk)
    got = ctx.gn_finalize(st0.cuda(), np0, G, EPS, mode, HW, st1=st1.cuda() if C1 else None, np1=np1, **kk).cpu()
    r = _ratio(got, want, 2e-5, gn_ref.gate_atol(mean, var, EPS, mode, C0 + C1, **rk))
    print(f"gn_finalize {name} mode {mode}: {r:.3g} x the gate")
    assert r <= 1.0, f"gn_finalize {name} mode {mode}: coefficients at {r:.3g} x the gate"
    # ... and those partials stand for the tensor
    _check_coef(got, x, shape, mode, rk, "gn_finalize vs the tensor")


def _gn_coef(ctx, x, shape, mode, kk):
    name, B, C0, C1, HW, G, np0, np1 = shape
    d = x.cuda()
    x0 = d[:, :C0].contiguous().view(B, C0, 1, HW)
    x1 = d[:, C0:].contiguous().view(B, C1, 1, HW) if C1 else None
    return ctx.gn_coef(x0, G, EPS, mode, x1=x1, **kk)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", REDUCER_SHAPES + COEF_EDGE_SHAPES, ids=lambda s: s[0])
def test_gn_coef_against_float64(ctx, shape, mode):
    x, emb, wgt, bia = _data(shape, "gauss")
    rk, kk = _mode_args(mode, emb, wgt, bia)
    _check_coef(_gn_coef(ctx, x, shape, mode, kk), x, shape, mode, rk, "gn_coef")


@pytest.mark.parametrize("kind", ["offset+40", "offset-300", "const"])
@pytest.mark.parametrize("shape", REDUCER_SHAPES + COEF_EDGE_SHAPES, ids=lambda s: s[0])
def test_gn_coef_data_kinds(ctx, shape, kind):
    x, emb, wgt, bia = _data(shape, kind)
    mode = 1 if kind == "offset+40" else 0
    rk, kk = _mode_args(mode, emb, wgt, bia)
    got = _gn_coef(ctx, x, shape, mode, kk)
    _check_coef(got, x, shape, mode, rk, f"gn_coef {kind}")
    if kind == "const":
        want_a = 1.0 / EPS ** 0.5
        assert ((got[..., 0].double().cpu() - want_a).abs() <= 1e-6 * want_a).all()


def outlier_group(gs, HW, value, where, B=2, G=3, seed=5):
    """[B, G * gs, HW] unit Gaussian with ONE element of every group replaced: the group's first (`where` = 0) or another."""
    x = torch.randn(B, G, gs * HW, generator=torch.Generator().manual_seed(seed))
    x[:, :, where] = value
    return x.view(B, G * gs, HW).contiguous()


@pytest.mark.parametrize("where", [0, 1777], ids=["outlier_first", "outlier_elsewhere"])
@pytest.mark.parametrize("value", [1e3, 3e4])
@pytest.mark.parametrize("gs,HW", [(4, 1024), (3, 4096)])
def test_gn_coef_with_an_outlier(ctx, gs, HW, value, where):
    """One element of a group far from the rest -- the [0, 0] corner of a zero-padded conv output is a group's first element.  With the
    group's first element as the pilot of a shifted one-pass variance this was the cancellation the pilot is there to prevent (rstd off by
    1.8e-4 .. 1.2e-3 in the emulation, tests/test_gn_ref_cpu.py); moments merged from per-float4 means do not care where it sits."""
    shape = ("outlier", 2, 3 * gs, 0, HW, 3, 1, 1)
    x = outlier_group(gs, HW, value, where)
    _check_coef(_gn_coef(ctx, x, shape, 0, {}), x, shape, 0, {}, f"gn_coef outlier {value:g} at {where}")
