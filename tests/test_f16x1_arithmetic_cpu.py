"""CPU: the one-piece fp16 Winograd arithmetic (conv_wino2h.cpp with NP = 1, option "f16x1") -- its fp64 restatement (tests/f16x1_ref.py) against
the bound derived there, and the addresses the kernel forms into the two-piece weight image it shares with conv_wino2h.cpp."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import f16x1_ref as R


def _data(kind, B, Cin, Cout, H, W, wmag, xmag, seed=7):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    if kind == "const":                      # constant planes: all but one transform position cancel to zero exactly
        x = torch.randn(B, Cin, 1, 1, generator=g).expand(B, Cin, H, W).contiguous() * 3.0
    elif kind == "cancel":                   # channel pairs carry the same plane under weights (w, -w (1 + 2^-12)): sums cancel, errors do not
        x[:, 1::2] = x[:, 0::2]
        w[:, 1::2] = -w[:, 0::2] * (1.0 + 2.0 ** -12)
    return x * xmag, w * wmag


@pytest.mark.parametrize("wmag,xmag", [(1.0, 1.0), (1e-3, 30.0), (40.0, 0.02)], ids=["unit", "small_w_big_x", "big_w_small_x"])
@pytest.mark.parametrize("kind", ["gauss", "const", "cancel"])
@pytest.mark.parametrize("B,Cin,Cout,H,W", [(2, 48, 32, 8, 8), (1, 96, 64, 16, 32)])
def test_restatement_meets_the_derived_bound(kind, wmag, xmag, B, Cin, Cout, H, W):
    """|y - y64| <= (2^-10 + 2^-22 + (16 K + 4) 2^-24) |A|^T [sum_c |U_c| (.) |V_c|] |A| + underflow term, per element, y64 the fp64
    convolution and K = Cin (tests/f16x1_ref.py derives it).  The UNDERFLOW term: a scaled operand u = U s or v = 16 V with
    0 < |.| < 2^-14 sits on the fixed 2^-24 grid of the fp16 subnormals, so its rounding error is bounded by 2^-25 instead of 2^-11 |.|;
    such a product contributes 2^-25 (1 + 2^-11) |other operand| (2^-50 when both are that small), carried through |A|^T . |A| and
    divided by 16 s like everything else.  Also: the bound is not vacuous (the error is within it but is NOT fp32-sized) and the per-layer
    scale makes the relative error independent of the magnitudes."""
    x, w = _data(kind, B, Cin, Cout, H, W, wmag, xmag)
    y, bound = R.wino_f16x1(x, w)
    y64 = F.conv2d(x.double(), w.double(), None, padding=1)
    err = (y - y64).abs()
    assert torch.isfinite(y).all()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"f16x1 restatement {kind} w*{wmag} x*{xmag} K{Cin}: worst |err| / bound = {ratio:.3f}, max|err| / max|y| = {err.max().item() / y64.abs().max().item():.2e}")
    assert (err <= bound).all(), ratio
    if kind == "gauss":
        rel = err.max().item() / y64.abs().max().item()
        assert 2e-5 < rel < 2e-3, rel        # an 11-bit arithmetic: far from fp32 (1e-7), far from broken


def test_bound_has_an_underflow_term_where_operands_are_subnormal(monkeypatch):
    """Inputs so small that 16 V falls below 2^-14: the relative term alone no longer covers the rounding, with the underflow term the
    bound holds."""
    x, w = _data("gauss", 1, 32, 32, 8, 8, 1.0, 2.0 ** -26)
    y, bound = R.wino_f16x1(x, w)
    y64 = F.conv2d(x.double(), w.double(), None, padding=1)
    err = (y - y64).abs()
    assert (err <= bound).all()
    monkeypatch.setattr(R, "F16_MIN_NORMAL", 0.0)               # no operand counts as subnormal: the relative term alone
    _, rel_only = R.wino_f16x1(x, w)
    assert (rel_only < bound).all() and (err > rel_only).any()


def test_weight_scale_rule():
    g = torch.Generator().manual_seed(3)
    for mag in (1e-4, 1.0, 300.0):
        w = torch.randn(8, 8, 3, 3, generator=g) * mag
        s = R.weight_scale(w)
        assert np.log2(s) == int(np.log2(s))
        assert 2.0 ** 13 <= 2.25 * float(w.abs().max()) * s < 2.0 ** 14


# ------------------------------------------------------------------------------------------------ addresses into the shared weight image
@pytest.mark.parametrize("COT,Cout,Cin,CinP", [(3, 192, 40, 48), (2, 128, 32, 32), (1, 64, 16, 16)])
def test_one_piece_loop_reads_exactly_the_first_pieces(COT, Cout, Cin, CinP):
    """conv_wino2h.cpp's one-piece form (NP = 1) reads the two-piece weight image [cout tile][chunk][position][cout sub-tile][piece][64 lanes][4 dwords]
    (pack_wino2h_weight_kernel, restated here halfword by halfword).  The addresses of H2_LOAD_A (QS = 512) -- per (cout tile, chunk, wave, position
    of the wave, cout sub-tile): 64 lanes x 4 dwords -- must hit every dword of every piece-0 quad exactly once and no dword of a piece-1
    quad; and what lands in the A-operand registers, contracted by the MFMA's K-slot convention with the ONE plane H2_WRITE_V parks
    (read back by H2_LOAD_B), must be the plain contraction over the chunk's channels."""
    rng = np.random.default_rng(0)
    BCO, CoutP, nch = 32 * COT, Cout, CinP // 16
    U = rng.standard_normal((Cout, CinP, 16))
    U[:, Cin:] = 0
    ndw = CinP * 16 * CoutP                                     # dwords of the image behind the header: two fp16 each, two pieces
    mem = np.zeros(ndw * 2)
    piece_of = np.full(ndw, -1)
    for co in range(Cout):
        for ci in range(CinP):
            cotile, ct, cc = co // BCO, (co % BCO) // 32, ci & 15
            h, el = cc & 1, cc >> 1
            lane = h * 32 + (co & 31)
            base = (((cotile * nch + (ci >> 4)) * 16) * COT + ct) * 1024 + (lane * 4 + (el >> 1)) * 2 + (el & 1)
            for xi in range(16):
                for p in range(2):
                    o = base + xi * COT * 1024 + p * 512
                    mem[o] = (1.0, 7.0)[p] * U[co, ci, xi]
                    piece_of[o // 2] = p
    assert (piece_of >= 0).all()
    hits = np.zeros(ndw, dtype=int)
    V = rng.standard_normal((16, 16, 32))                       # [channel in chunk][position][tile]
    sV = np.zeros((16 * 2 * 4 * 32, 2))                         # H2_WRITE_V, NP = 1: words [position][half][pair][tile] = (lo, hi)
    for tid in range(512):
        rg, s_tile, s_cp = (tid >> 6) >> 2, tid & 31, (tid & 255) >> 5
        s_ca = 4 * (s_cp >> 1) + (s_cp & 1)
        v_wr = ((8 * rg * 2 + (s_cp & 1)) * 4 + (s_cp >> 1)) * 32 + s_tile
        for row in range(2):
            for q in range(4):
                xi = (2 * rg + row) * 4 + q
                sV[v_wr + (row * 4 + q) * 256] = (V[s_ca, xi, s_tile], V[s_ca + 2, xi, s_tile])
    for cotile in range(Cout // BCO):
        for chunk in range(nch):
            for wave in range(8):
                for i in range(2):
                    xi = 2 * wave + i
                    for ct in range(COT):
                        A, Bm = np.zeros((32, 2, 8)), np.zeros((32, 2, 8))
                        for lane in range(64):
                            half, l31 = lane >> 5, lane & 31
                            q = i * COT + ct                                            # H2_LOAD_A / H2_MF1, NP = 1: quad of (position, sub-tile)
                            dw0 = (cotile * nch * 16 + 2 * wave) * (COT * 512) + chunk * (16 * COT * 512) + q * 512 + lane * 4
                            hits[dw0:dw0 + 4] += 1
                            A[l31, half] = [mem[(dw0 + j) * 2 + k] for j in range(4) for k in range(2)]
                            qb = (((2 * wave + i) * 2 + half) * 4) * 32 + l31           # H2_LOAD_B, NP = 1
                            Bm[l31, half] = [sV[qb + jp * 32][k] for jp in range(4) for k in range(2)]
                        if chunk == nch - 1:
                            co0 = cotile * BCO + ct * 32
                            want = np.einsum("mc,cn->mn", U[co0:co0 + 32, chunk * 16:chunk * 16 + 16, xi], V[:, xi, :])
                            assert np.allclose(np.einsum("mhe,nhe->mn", A, Bm), want), (cotile, wave, i, ct)
    assert (hits[piece_of == 0] == 1).all(), "a first-piece dword is read twice or never"
    assert (hits[piece_of == 1] == 0).all(), "the one-piece loop reads a second piece"
