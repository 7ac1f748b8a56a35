"""CPU: the float64 restatement of GroupNorm (tests/gn_ref.py) against torch and the oracle, the fold of partials against the tensor's own
moments, the GPU test's case table against the id table of conv_kernels.h, and an emulation of gn_coef_kernel's fp32 arithmetic that shows
the `outlier_first` data kind separates a one-pilot shifted variance from merged moments.
"""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import unet_ref
from tests import gn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcvd_pytorch_amd", "csrc")
D = torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _partials(x, np_, perm=None):
    """[B, C, HW] float64 -> [B, C, np, 2] over np equal parts of the plane; `perm` reorders the pixels first (any partition will do)."""
    B, C, HW = x.shape
    if perm is not None:
        x = x[:, :, perm]
    xp = x.view(B, C, np_, HW // np_)
    return torch.stack([xp.sum(-1), ((xp - xp.mean(-1, keepdim=True)) ** 2).sum(-1)], -1)


# (B, C0, C1, H, groups, np0, np1)
NORM_SHAPES = [
    (2, 96, 0, 8, 24, 2, 1),
    (3, 64, 32, 8, 32, 4, 1),          # a concat, the seam on a group boundary
    (2, 40, 44, 8, 4, 2, 64),          # 21 channels per group, the seam (40) inside group 1
    (2, 2304, 0, 4, 32, 1, 1),         # 72 channels per group
    (2, 1188, 1116, 4, 32, 16, 2),     # ... with the seam in the middle of group 16
]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", NORM_SHAPES, ids=lambda s: "c{}+{}_H{}_g{}".format(s[1], s[2], s[3], s[4]))
@pytest.mark.parametrize("src", ["tensor", "partials"])
def test_restatement_is_group_norm(shape, mode, src):
    B, C0, C1, H, G, np0, np1 = shape
    C, HW = C0 + C1, H * H
    g = _g(3)
    x = torch.randn(B, C, H, H, generator=g, dtype=D) * (0.5 + torch.rand(B, C, 1, 1, generator=g, dtype=D)) + torch.randn(B, C, 1, 1, generator=g, dtype=D)
    eps = 1e-5
    emb = torch.randn(B, 2 * C + 9, generator=g, dtype=D)
    wgt, bia = 1 + 0.1 * torch.randn(C, generator=g, dtype=D), 0.1 * torch.randn(C, generator=g, dtype=D)
    x0, x1 = x[:, :C0], x[:, C0:]
    if src == "tensor":
        sources = [("tensor", x0)] + ([("tensor", x1)] if C1 else [])
    else:
        sources = [("partials", _partials(x0.flatten(2), np0))] + ([("partials", _partials(x1.flatten(2), np1))] if C1 else [])
    mean, var = gn_ref.group_moments(sources, HW, G)
    kw = {1: dict(p0=emb, emb_off=5), 2: dict(p0=wgt, p1=bia)}.get(mode, {})
    coef = gn_ref.coefficients(mean, var, eps, mode, C, **kw)
    assert coef.dtype == D and coef.shape == (B, C, 2)
    got = x * coef[..., 0][:, :, None, None] + coef[..., 1][:, :, None, None]
    plain = F.group_norm(x, G, eps=eps)
    assert (unet_ref.group_norm_plain(x, G, eps) - plain).abs().max().item() <= 1e-12
    if mode == 1:
        want = plain * (1 + emb[:, 5:5 + C, None, None]) + emb[:, 5 + C:5 + 2 * C, None, None]
    elif mode == 2:
        want = F.group_norm(x, G, weight=wgt, bias=bia, eps=eps)
    else:
        want = plain
    assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
    # the gate's absolute part is 2e-6 where |mean * rstd * par0| <= 1 and grows with it
    atol = gn_ref.gate_atol(mean, var, eps, mode, C, **kw)
    assert atol.shape == (B, C, 1) and (atol >= 2e-6).all()


@pytest.mark.parametrize("np_", [1, 2, 8, 32, 256])
def test_fold_of_any_equal_partition_gives_the_tensors_moments(np_):
    g = _g(4)
    B, C, HW = 3, 7, 1024
    x = torch.randn(B, C, HW, generator=g, dtype=D) * 3 + 40 * torch.randn(B, C, 1, generator=g, dtype=D)
    want_sum, want_m2 = gn_ref.tensor_moments(x)
    for perm in (None, torch.randperm(HW, generator=g)):
        s, m2 = gn_ref.fold_partials(_partials(x, np_, perm), HW)
        assert (s - want_sum).abs().max().item() <= 1e-12 * want_sum.abs().max().item()
        assert (m2 - want_m2).abs().max().item() <= 1e-12 * want_m2.abs().max().item()


# ------------------------------------------------------------------------------------------------ the id table
def _header_rows():
    """{id: (family, kparts)} parsed from kConvKernels."""
    src = open(os.path.join(CSRC, "conv_kernels.h")).read()
    enum = dict((n, int(v)) for n, v in re.findall(r"\b(CK_\w+) = (-?\d+)", src))
    body = src[src.index("kConvKernels[] = {"):src.index("kNoConvKernel")]
    rows = {}
    for name, fam, kp in re.findall(r"\{(CK_\w+),\s*\"\w+\",\s*CF_(\w+),\s*\d+,\s*\d+,\s*(\d+),", body):
        rows[enum[name]] = (fam, int(kp))
    return rows


def test_every_kernel_id_has_a_statistics_case_or_a_reason():
    from tests import test_gpu_gn_partials as T
    rows = _header_rows()
    assert len(rows) >= 26 and rows[10] == ("WINO3", 0) and rows[27] == ("WINO1H", 4)
    assert rows == gn_ref.KERNELS, "tests/gn_ref.py: KERNELS is not the table of conv_kernels.h"
    emitting = {c[0] for c in T.CASES if gn_ref.expected_np(c[0], c[5], c[5], c[1]) > 0}
    for kid in rows:
        in_cases, excused = kid in emitting, kid in T.DOES_NOT_EMIT
        assert in_cases != excused, f"id {kid}: {'both an emitting case and an excuse' if in_cases else 'neither a statistics case nor a reason in DOES_NOT_EMIT'}"
        if excused:
            assert T.DOES_NOT_EMIT[kid] and all(gn_ref.expected_np(kid, h, h) == 0 for h in (8, 16, 32, 64, 128))
    assert set(T.DOES_NOT_EMIT) <= set(rows)
    assert len(set(map(T._case_id, T.CASES))) == len(T.CASES), "two cases share a name"
    # every case asks for a shape its id can run: K parts divide the chunks, the 1x1 GEMMs get whole 16-channel chunks
    for kid, B, C0, C1, Cout, H, kind, cot, pgrid in T.CASES:
        fam, kp = rows[kid]
        assert (C0 + C1) % 16 == 0 or fam == "TILE"
        assert kp == 0 or ((C0 + C1) // 16) % kp == 0


def test_expected_np_restates_the_launchers():
    src = lambda f: open(os.path.join(CSRC, "kernels", f)).read()
    # the Winograd launchers end in one shared tail (conv_wino.cpp: wino_launch_done), each with its own geometry; the persistent kernel: regions only
    assert "if (a.stats) set_last_conv_stats_np(g8 ? 1 : (a.H / 8) * (a.W / 16));" in src("conv_wino.cpp")
    for f in ("conv_wino.cpp", "conv_wino2h.cpp", "conv_wino3.cpp"):          # conv_wino2h.cpp: one launch chain for both piece counts
        assert "wino_launch_done(a, G8, ksp, s)" in src(f) and src(f).count("wino_launch_done(") == (2 if f == "conv_wino.cpp" else 1), f      # (conv_wino.cpp defines it)
    assert "return wino_launch_done(a, false, ksp, s);" in src("conv_wino3p.cpp") and "set_last_conv_stats_np" not in src("conv_wino3p.cpp")
    assert src("conv1x1_dma.cpp").count("set_last_conv_stats_np(a.H * a.W / 32)") == 2
    assert "(HW >= Q1_PT || HW == 64)) set_last_conv_stats_np(HW >= Q1_PT ? HW / Q1_PT : 1)" in src("conv1x1_h2.cpp")
    assert re.search(r"constexpr int Q1_PT = 128;", src("conv1x1_h2.cpp"))
    assert "if (!SPLIT && a.stats && g.nimg == 1) set_last_conv_stats_np(a.H * a.W / (PXT * 32))" in src("conv_mfma.h")
    w = src("conv_wino.cpp")
    assert w.count("set_last_conv_stats_np(1)") == 2 and "if (a.stats) set_last_conv_stats_np(0)" in w
    assert "(hw4 == 16 || hw4 == 64)" in src("gn.cpp")
    e = gn_ref.expected_np
    assert [e(10, 8, 8), e(10, 16, 16), e(10, 32, 32), e(16, 64, 64)] == [1, 2, 8, 32]
    assert [e(11, 8, 8), e(19, 16, 16), e(26, 32, 32)] == [1, 1, 0]
    assert [e(5, 8, 8), e(9, 16, 16), e(15, 8, 8), e(14, 16, 16), e(15, 64, 64)] == [2, 8, 1, 2, 32]
    assert [e(0, 8, 8), e(0, 16, 16), e(0, 64, 64), e(1, 8, 8), e(1, 16, 16), e(1, 64, 64), e(2, 64, 64), e(3, 16, 16)] == [0, 4, 64, 0, 8, 128, 0, 0]


# ------------------------------------------------------------------------------------------------ does the data kind tell right from wrong?
def _gate_ratio(mean, rstd, x, eps):
    """The section-4 gate on the mode-0 pair (A, B) = (rstd, -mean * rstd) of one group, float64 reference."""
    d = np.asarray(x, np.float64)
    wm, wr = d.mean(), 1.0 / np.sqrt(d.var() + eps)
    atol = 2e-6 * max(1.0, abs(wm * wr))
    ra = abs(float(rstd) - wr) / (2e-5 * wr + atol)
    rb = abs(-float(mean) * float(rstd) + wm * wr) / (2e-5 * abs(wm * wr) + atol)
    return max(ra, rb)


@pytest.mark.parametrize("value", [1e3, 3e4])
@pytest.mark.parametrize("gs,HW", [(4, 1024), (3, 4096)])
def test_outlier_first_separates_one_pilot_from_merged_moments(gs, HW, value):
    x = np.random.default_rng(9).standard_normal(gs * HW).astype(np.float32)
    first, elsewhere = x.copy(), x.copy()
    first[0] = value
    elsewhere[1777] = value
    eps = 1e-5
    bad = _gate_ratio(*gn_ref.emulate_gn_coef_pilot(first, eps), first, eps)
    assert bad > 1.0, f"one pilot = the outlier: {bad:.3g} x the gate (expected to miss it)"
    assert _gate_ratio(*gn_ref.emulate_gn_coef_pilot(elsewhere, eps), elsewhere, eps) <= 1.0
    for data in (first, elsewhere):
        r = _gate_ratio(*gn_ref.emulate_gn_coef_merge(data, eps), data, eps)
        assert r <= 1.0, f"merged moments: {r:.3g} x the gate"


@pytest.mark.parametrize("n4", [4, 16, 64, 255, 256, 257, 511, 512, 513, 1300])
def test_emulations_visit_every_element_once(n4):
    """Both emulations walk the kernel's two-stream loop: on easy data they agree with float64 at fp32 accuracy for every loop edge."""
    x = (np.random.default_rng(n4).standard_normal(4 * n4) * 2 + 3).astype(np.float32)
    d = x.astype(np.float64)
    for f in (gn_ref.emulate_gn_coef_pilot, gn_ref.emulate_gn_coef_merge):
        mean, rstd = f(x, 1e-5)
        assert abs(float(mean) - d.mean()) <= 2e-6 and abs(float(rstd) * np.sqrt(d.var() + 1e-5) - 1) <= 2e-6, f.__name__
