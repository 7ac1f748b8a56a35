"""CPU: the case lists of tests/test_gpu_conv_paths.py cover every id the dispatcher launches, and the id each case expects follows from
tests/wino_rule.admits and the fallback lists of conv_kernels.h; the float64 restatement of tests/conv_ref.py is F.conv2d's."""
import os
import re

import torch
import torch.nn.functional as F

from tests import conv_ref as CR
from tests import test_gpu_conv_paths as G
from tests import wino_rule as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "mcvd_pytorch_amd", "csrc", "kernels")


def test_every_dispatcher_id_is_in_both_parts():
    table = CR.kernel_table()
    ids = CR.dispatcher_ids()
    assert ids == [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 24, 25, 26, 27], ids
    assert set(table) - set(ids) == {22, 23}
    one = {c.kid for _, c in G.PART_ONE}
    assert set(G.IDS3 + G.IDS1) | {k for k, _ in G.KSPLIT_MIN} <= one, one
    # part two: every id on every plane, and the id itself runs on at least one of them
    for kid in ids:
        planes = {(c.H, c.W) for p, c in G.PART_TWO if c.kid == kid and p == "plane"}
        assert set(G.PLANES) <= planes, (kid, planes)
        assert any(CR.expected_id(c, table) == kid for p, c in G.PART_TWO if c.kid == kid), kid
        if table[kid][0] in G.KS1:
            assert {c.B for p, c in G.PART_TWO if c.kid == kid and (c.H, c.W) == (4, 8) and p == "plane"} == {4, 5, 6}, kid
    for kid in G.BIT_EQUAL:
        assert {c.pgrid for p, c in G.PART_TWO if c.kid == kid and (c.H, c.W) == (8, 16)} == {0, 1, 7}, kid
    # every gate class has its ids, and no dispatcher id is without one
    classes = G.FP32_IDS + G.THREE + G.TWO_WINO + G.TWO_1X1 + G.ONE + tuple(G.BIT_EQUAL) + G.NEAR_10
    assert sorted(classes) == ids
    for kid, base in list(G.FP32_BASE.items()) + list(G.BIT_EQUAL.items()):
        assert table[kid][1] == table[base][1] and (table[kid][3] != 0) == (table[base][3] != 0), (kid, base)      # kernel size; split or not
    # the paths of part one, on Gaussian data, and the structured kinds for one id per arithmetic
    for kid in G.IDS3:
        paths = {p for p, c in G.PART_ONE if c.kid == kid and c.kind == "gauss"}
        assert {"raw", "affine", "silu", "concat", "cout5", "g8"} <= paths, (kid, paths)
        assert ("ragged" in paths) == (table[kid][3] == 0), (kid, paths)           # three chunks do not split
    for kid in G.IDS1:
        paths = {p for p, c in G.PART_ONE if c.kid == kid and c.kind == "gauss"}
        assert {"raw", "affine", "silu", "concat", "ragged", "cout40", "g8"} <= paths, (kid, paths)
        assert {c.B for p, c in G.PART_ONE if c.kid == kid and p == "g8"} == {3, 5}
    for kid in G.KINDS_IDS:
        assert {(p, c.kind) for p, c in G.PART_ONE if c.kid == kid and c.kind != "gauss"} == {
            (p, k) for p in ("silu", "concat") for k in ("const", "dominant", "cancel")}, kid


def test_the_expected_id_agrees_with_the_admission_rule_on_every_case():
    table = CR.kernel_table()
    n_wino = 0
    for path, c in G.PART_ONE + G.PART_TWO:
        want = CR.expected_id(c, table)
        fam0, _, _, kp0, _, wt0, fallback = table[c.kid]
        CinP, cot, CoutP = CR.launch_geometry(c)
        assert CinP % (16 if c.ks == 3 else 32) == 0 and CoutP % (32 * cot) == 0 and CoutP >= c.Cout
        if fam0 in CR.WINO_FAMILIES:
            assert c.ks == 3
            n_wino += 1
            room = kp0 * c.B * c.Cout * c.H * c.W
            verdict = [WR.admits(table[k][0], c.C0 + c.C1, CinP, WR.kernel_parts(table[k][0], table[k][3] if k != 4 else 0), (c.H, c.W), C0=c.C0, B=c.B,
                                 Cout=c.Cout, CoutP=CoutP, weights=table[k][5] in (wt0, "CW_WPW"), part_floats=room) for k in fallback]
            if want == "direct":
                assert not any(verdict), (c, verdict)
            else:
                i = fallback.index(want)
                assert verdict[i] and not any(verdict[:i]), (c, want, verdict)
        elif fam0 == "TILE":
            assert fallback == [] and (want == c.kid) == CR.tile_fits(c.kid, c), (c, want)
        else:
            assert fallback == [c.kid] and want in (c.kid, "direct"), (c, want)
        if path == "plane" and (c.H, c.W) in G.PLANES and fam0 != "TILE" and (c.kid, (c.H, c.W), "direct") not in G.REFUSED:
            assert want == c.kid, (c, want)                   # every plane of the list is admitted at the id's own smallest Cin
    assert n_wino > 100
    # the refusals of part two, spelled out
    for kid, plane, must in G.REFUSED:
        cs = [c for p, c in G.PART_TWO if c.kid == kid and (c.H, c.W) == plane and c.B == 3]
        assert cs and all(CR.expected_id(c, table) == must for c in cs), (kid, plane, must)
    # every admitted plane of part two is one the header's list admits for the family, every refused one is refused there
    header = {(f, h, w): ad for f, h, w, parts, cin, ad in WR.header_plane_cases() if parts == 1}
    for plane in G.PLANES:
        assert header[("WINO3", plane[0], plane[1])] is True, plane
    assert header[("WINO3", 12, 16)] is False and header[("WINO3", 16, 8)] is False and header[("WINO3P", 8, 8)] is False


def test_the_1x1_predicates_are_the_kernels():
    """The constants and clauses conv_ref restates, found in the kernel files."""
    h2 = open(os.path.join(KERNELS, "conv1x1_h2.cpp")).read()
    dma = open(os.path.join(KERNELS, "conv1x1_dma.cpp")).read()
    consts = dict(re.findall(r"constexpr int (Q1_PT|Q1_CK|Q1_NB|Q1_MAXIMG) = (\d+);", h2))
    assert {k: int(v) for k, v in consts.items()} == dict(Q1_PT=CR.Q1_PT, Q1_CK=CR.Q1_CK, Q1_NB=CR.Q1_NB, Q1_MAXIMG=CR.Q1_MAXIMG), consts
    consts = dict(re.findall(r"constexpr int (G1_PT|G1_MAXIMG) = (\d+);", dma))
    assert {k: int(v) for k, v in consts.items()} == dict(G1_PT=CR.G1_PT, G1_MAXIMG=CR.G1_MAXIMG), consts
    assert "if (!(HW % Q1_PT == 0 || (HW < Q1_PT && Q1_PT % HW == 0 && Q1_PT / HW <= Q1_MAXIMG))) return false;" in h2
    assert "return q1_lds_bytes(np, cot, a.Cin, HW, a.coef != nullptr) <= 80 * 1024;" in h2
    assert "if (!(HW % PT == 0 || (HW < PT && PT % HW == 0 && PT / HW <= G1_MAXIMG))) return false;" in dma
    assert "if (a.Cin % G1_CK != 0 || a.CinP % G1_CK != 0) return false;" in dma
    c = CR.case
    assert CR.split1_supported(c(15, 1, 4, 64, 0, 40, (4, 8)), 1, 3) and not CR.split1_supported(c(15, 1, 4, 64, 0, 40, (2, 8)), 1, 3)
    assert CR.dma1_supported(c(5, 1, 4, 64, 0, 40, (4, 8)), 16, 1) and not CR.dma1_supported(c(9, 1, 4, 64, 0, 40, (4, 8)), 16, 2)
    assert CR.dma1_supported(c(9, 1, 3, 64, 0, 40, 8), 16, 2) and not CR.dma1_supported(c(6, 1, 3, 80, 0, 40, 8), 32, 1)
    assert not CR.split1_supported(c(15, 1, 3, 72, 0, 64, 16), 2, 3) and not CR.split1_supported(c(15, 1, 3, 64, 0, 96, 16), 2, 3)


def _keep_bits(t, bits):
    """Round to `bits` significant bits (what an operand keeps when its low-order piece is dropped)."""
    m, e = torch.frexp(t.double())
    return torch.ldexp(torch.round(m * 2.0 ** bits) / 2.0 ** bits, e).float()


def _cpu_stand_in(slip):
    """A _run for measure(): the case in plain float32 on the CPU, reporting the expected id; `slip` puts one subtle mistake in."""
    def run(ctx, c):
        t = CR.inputs(c)
        x = torch.cat([t["x0"], t["x1"]], 1) if t["x1"] is not None else t["x0"]
        if c.coef:
            x = t["coef"][..., 0][:, :, None, None] * x + t["coef"][..., 1][:, :, None, None]
        if c.act:
            x = x / (1 + torch.exp(-x))
        w, res = t["w"], t["res"]
        if slip == "dropped piece" and c.kid in G.THREE:
            x, w = _keep_bits(x, 16), _keep_bits(w, 16)            # two bf16 pieces of three
        if slip == "residual rounded" and c.res:
            res = _keep_bits(res, 16)
        y = F.conv2d(x, w, t["bias"], padding=c.ks // 2)
        if c.res:
            y = (y + res) * t["scale"]
        want = CR.expected_id(c, G.TABLE)
        return (2 if want == "direct" else want), y, True, None
    return run


def test_the_gates_pass_a_float32_evaluation_and_catch_a_dropped_piece(monkeypatch):
    """measure() and check() over a CPU stand-in for the kernels: plain float32 meets every gate; operands of 16 bits (the third bf16 piece
    dropped: 2^-17 of a term) miss the three-piece gate on every path and plane, a residual rounded once too often misses the fp32 one."""
    cases = [(p, c._replace(stats=False)) for p, c in G.PART_ONE + G.PART_TWO if c.kid in (4, 5, 10, 15, 11) and c.kind in ("gauss", "cancel")]
    assert len(cases) > 80
    monkeypatch.setattr(G, "_run", _cpu_stand_in(None))
    worst = 0.0
    for _, c in cases:
        r = G.measure(None, c)
        G.check(c, r)
        worst = max(worst, r["err"])
    assert worst < 5e-7, worst                                # the reference arithmetic itself leaves a factor 4 below 2e-6
    for slip, ids in (("dropped piece", G.THREE), ("residual rounded", (4, 5))):
        monkeypatch.setattr(G, "_run", _cpu_stand_in(slip))
        caught = missed = 0
        for _, c in cases:
            if c.kid not in ids or (slip == "residual rounded" and not c.res):
                continue
            r = G.measure(None, c)
            try:
                G.check(c, r)
                missed += 1
            except AssertionError:
                caught += 1
        assert caught > 10 and missed == 0, (slip, caught, missed)


def test_the_float64_restatement_is_conv2d_and_the_kinds_are_the_parity_files():
    from tests import test_gpu_parity as P
    c = CR.case(10, 3, 3, 48, 16, 40, (8, 16), res=True, kind="cancel")
    t = CR.inputs(c)
    assert t["x0"].shape == (3, 48, 8, 16) and t["x1"].shape == (3, 16, 8, 16) and t["res"].shape == (3, 40, 8, 16) and t["scale"] == 0.70710678
    x = torch.cat([t["x0"], t["x1"]], 1)
    assert torch.equal(x[:, 1::2], x[:, 0::2]) and torch.equal(t["coef"][:, 1::2], t["coef"][:, 0::2])
    assert torch.equal(t["w"][:, 1::2], -t["w"][:, 0::2] * (1.0 + 2.0 ** -12))
    xin = t["coef"][..., 0][:, :, None, None] * x + t["coef"][..., 1][:, :, None, None]
    xin = xin * torch.sigmoid(xin)
    want32 = (F.conv2d(xin, t["w"], t["bias"], padding=1) + t["res"]) * t["scale"]
    err = (want32.double() - CR.reference(c)).abs().max().item() / CR.mag(c)
    assert err < 2e-6, err                                    # a plain fp32 evaluation meets the gate the kernels are held to
    assert CR.mag(c) >= CR.reference(c).abs().max().item()
    assert CR.reference(c) is CR.reference(c._replace(kid=4, pgrid=7))             # computed once, shared
    # the data kinds are test_gpu_parity's, generator call for generator call, on a square plane
    for kind in ("gauss", "const", "dominant", "cancel"):
        a = CR.structured(kind, 2, 8, 4, 4, torch.Generator().manual_seed(3))
        b = P._structured(kind, 2, 8, 4, torch.Generator().manual_seed(3))
        assert torch.equal(a, b), kind
    w = torch.randn(4, 8, 3, 3, generator=torch.Generator().manual_seed(4))
    assert torch.equal(CR.pair_weights(w), P._pair_weights(w))
    # the one-piece bound covers a float64 evaluation of its own restatement's error on a non-square plane
    c1 = CR.case(24, 3, 2, 64, 0, 40, (8, 32), res=True)
    assert CR.f16x1_bound(c1).shape == CR.reference(c1).shape and (CR.f16x1_bound(c1) > 0).all()
