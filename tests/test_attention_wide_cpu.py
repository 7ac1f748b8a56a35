"""CPU: the wide-head attention kernel's bookkeeping (mcvd_pytorch_amd/csrc/kernels/attention_wide.cpp) and the dispatch table in front of it
(attn_kernels.h), restated in Python and walked over every head dim D = 160 ... 1024 in steps of 32.

The kernel: a workgroup is AW_NW = 8 waves and one tile of 32 queries; wave w owns channel tiles [f_w, f_w + n_w) of the DT = D / 32 tiles of
the head, n_w = DT / NW + (w < DT % NW), f_w = w (DT / NW) + min(w, DT % NW).  Its K, Q and V operands are loaded from global memory in MFMA
operand order and split in the lane that feeds them to the matrix pipe -- no K / V tile is staged in the LDS, so the "staged tile" whose
slots are checked here is the operand image itself: (step, lane, dword, half-word) of every piece.
  S product  (v_mfma 32x32x16, A = K, B = Q): lane = key / query l31 + 32 h; step st, dword j, half-word e <-> slice channel 16 st + 4 j + 2 e + h
  PV product (A = V, B = P): lane = channel / query l31 + 32 h; step s2, dword j = 2 g + i, half-word e <-> key 16 s2 + 8 g + 4 h + 2 i + e,
      and P's element comes from accumulator register r = 8 s2 + 2 j + e of the S^T tile, whose row (the key) is (r & 3) + 8 (r >> 2) + 4 h.
The partial S^T tiles go through the LDS image [buffer t & 1][wave][quad q][64 lanes][4 dwords] (register r = 4 q + dword).
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcvd_pytorch_amd", "csrc")

NW = 8
D_MIN, D_MAX = 160, 1024
XCH = 1024                       # dwords of one wave's partial in the exchange image
TW_MAX = 4                       # launcher cases AW_CASE(1) ... AW_CASE(4)
DIMS = list(range(D_MIN, D_MAX + 1, 32))

AK_NAIVE, AK_FLASH_F32, AK_SPLIT2, AK_SPLIT3, AK_SPLIT3_PRESPLIT, AK_WIDE2, AK_WIDE3 = range(7)
AK_SPLIT_D_MAX, AK_F32_D_MAX, AK_WIDE_D_MIN, AK_WIDE_D_MAX = 128, 256, 160, 1024


def _src(*p):
    return open(os.path.join(CSRC, *p)).read()


def _const(src, name):
    m = re.search(r"constexpr int [^;]*\b%s = (\d+)[,;]" % name, src)
    assert m, name
    return int(m.group(1))


# ---- the kernel's expressions
def slices(DT):
    """[(first tile, tiles)] per wave."""
    tb, tr = DT // NW, DT % NW
    return [(w * tb + min(w, tr), tb + (1 if w < tr else 0)) for w in range(NW)]


def s_channel(st, j, e, h):
    """slice channel of half-word e of dword j, step st, lane half h: K (lane = key) and Q (lane = query) alike."""
    return 16 * st + 4 * j + 2 * e + h


def v_key(s2, j, e, h):
    """key of half-word e of dword j, step s2 of the V operand: the float4 at keys 16 s2 + 8 g + 4 h is dwords (2g, 2g + 1)."""
    g, i = j >> 1, j & 1
    return 16 * s2 + 8 * g + 4 * h + 2 * i + e


def p_key(s2, j, e, h):
    """key whose probability is half-word e of dword j, step s2 of the P operand: accumulator register r of the S^T tile."""
    r = 8 * s2 + 2 * j + e
    return (r & 3) + 8 * (r >> 2) + 4 * h


def xch_slot(buf, nwa, w, q, lane):
    """first dword of the 16-byte exchange slot."""
    return 4 * (buf * nwa * 256 + (w * 4 + q) * 64 + lane)


def test_the_restated_constants_are_the_kernels():
    src = _src("kernels", "attention_wide.cpp")
    assert _const(src, "AW_NW") == NW
    assert _const(src, "AW_D_MIN") == D_MIN and _const(src, "AW_D_MAX") == D_MAX
    assert _const(src, "AW_XCH") == XCH
    assert "const int tb = DT / AW_NW, tr = DT - tb * AW_NW;" in src
    assert "const int nt = tb + (wave < tr ? 1 : 0);" in src and "const int ft = wave * tb + min(wave, tr);" in src
    # Q and K: row 16 step + 4 j + half and that row + 2, lane l31 -- one expression for both
    assert "const float* qc = qb + (long)(16 * st + 4 * j) * S + q0;" in src and "qc[half * S + l31]" in src and "qc[half * S + l31 + 2 * S]" in src
    assert src.count("const float* kc = kt + (long)(16 * s + 4 * j) * S;") == 2          # the prefetch and the in-place load
    assert "klane = half * S + l31, klane2 = klane + 2 * S;" in src and "kr[PF ? s : 0][2 * j] = kc[klane];" in src and "kr[PF ? s : 0][2 * j + 1] = kc[klane2];" in src
    # V: row l31 of the tile, float4 at keys 16 s2 + 8 g + 4 half; the prefetch keeps it at [2 s2 + g]
    assert "vlane = l31 * S + 4 * half;" in src and "vt + (long)ct * 32 * S + 16 * s2 + 8 * g + vlane" in src
    assert "vt + (long)ct * 32 * S + 16 * (i >> 1) + 8 * (i & 1) + vlane" in src and "vr[PF ? ct : 0][2 * s2 + g]" in src
    assert "if (t + 1 < ntiles) kload(t + 1);" in src                        # no prefetch past the last key tile
    assert "PX::template split<false>(st[8 * s2 + 2 * j], st[8 * s2 + 2 * j + 1], w);" in src
    assert "xb[(wave * 4 + q) * 64 + lane]" in src and "sX + (t & 1) * nwa * 256" in src and "xb[(w * 4 + q) * 64 + lane]" in src
    assert "const int c = ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;" in src
    assert "for (int w = 1; w < nwa; ++w) a +=" in src                       # the partials are added in wave order
    assert re.search(r"AW_CASE\(1\) AW_CASE\(2\) AW_CASE\(3\) AW_CASE\(4\)\s*\}", src)
    assert "2 * (DT < AW_NW ? DT : AW_NW) * AW_XCH * sizeof(unsigned)" in src
    assert not re.search(r"atomic\w*\s*\(|__hip_atomic|std::atomic", src)      # a fixed order of additions, nothing else


def test_every_channel_belongs_to_exactly_one_wave():
    for D in DIMS:
        DT = D // 32
        owner = [None] * D
        sl = slices(DT)
        assert -(-DT // NW) <= TW_MAX
        for w, (ft, nt) in enumerate(sl):
            assert 0 <= nt <= -(-DT // NW) and 0 <= ft and ft + nt <= DT, (D, w)
            assert (nt == 0) == (w >= min(NW, DT)), (D, w)                    # the waves with channels are 0 ... NWA - 1: the ones the sum walks
            for c in range(32 * ft, 32 * (ft + nt)):                          # Q, K, V read and O written at head channel 32 ft + slice channel
                assert owner[c] is None, (D, c)
                owner[c] = w
        assert all(o is not None for o in owner), D
        assert [o for o in owner] == sorted(owner), D                         # contiguous slices in wave order


def test_operand_slots_cover_a_slice_once_and_pair_up():
    for nt in range(1, TW_MAX + 1):
        # S product: over (step, dword, half-word, lane half) every slice channel once; K and Q use the same map, so the contraction pairs
        # K[c] with Q[c]; the guard (st >> 1) < nt keeps exactly the steps of the wave's tiles
        seen = {}
        for st in range(2 * TW_MAX):
            if (st >> 1) >= nt:
                continue
            for j in range(4):
                for e in range(2):
                    for h in range(2):
                        c = s_channel(st, j, e, h)
                        assert c not in seen, (nt, st, j, e, h)
                        seen[c] = (st, j, e, h)
        assert sorted(seen) == list(range(32 * nt)), nt
    # the kernel loads the pair (c0, c0 + 2) into one dword: half-words 0 and 1
    for st in range(2):
        for j in range(4):
            for h in range(2):
                assert s_channel(st, j, 1, h) == s_channel(st, j, 0, h) + 2
    # PV product: every key of the tile once per lane half pair, and V's key is the key of the probability it meets
    for h in range(2):
        keys = []
        for s2 in range(2):
            for j in range(4):
                for e in range(2):
                    assert v_key(s2, j, e, h) == p_key(s2, j, e, h), (s2, j, e, h)
                    keys.append(v_key(s2, j, e, h))
        assert len(set(keys)) == 16
    both = sorted(v_key(s2, j, e, h) for h in range(2) for s2 in range(2) for j in range(4) for e in range(2))
    assert both == list(range(32))
    # the float4 loads: 4-key aligned, inside the tile
    for s2 in range(2):
        for g in range(2):
            for h in range(2):
                k0 = 16 * s2 + 8 * g + 4 * h
                assert k0 % 4 == 0 and k0 + 3 < 32
                assert [v_key(s2, 2 * g + i, e, h) for i in range(2) for e in range(2)] == [k0, k0 + 1, k0 + 2, k0 + 3]
    # output rows: accumulator register r of lane half h of tile ct -> slice channel, each once
    for ct in range(TW_MAX):
        rows = sorted(ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * h for r in range(16) for h in range(2))
        assert rows == list(range(32 * ct, 32 * ct + 32))


def test_exchange_slots_are_disjoint_and_fit():
    for D in DIMS:
        DT = D // 32
        nwa = min(NW, DT)
        lds_bytes = 2 * nwa * XCH * 4
        assert lds_bytes <= 64 * 1024 <= 160 * 1024, D
        used = set()
        for buf in range(2):
            for w in range(nwa):
                for q in range(4):
                    for lane in range(64):
                        s = xch_slot(buf, nwa, w, q, lane)
                        assert s % 4 == 0 and 0 <= s and (s + 4) * 4 <= lds_bytes, (D, buf, w, q, lane)
                        assert s not in used
                        used.add(s)
        assert len(used) * 16 == lds_bytes, D                                 # and nothing is left over
        # a reader finds register r = 4 q + e of wave w at dword e of slot (w, q, its own lane): one wave's partial is XCH dwords
        assert xch_slot(0, nwa, 1, 0, 0) - xch_slot(0, nwa, 0, 0, 0) == XCH
        assert xch_slot(1, nwa, 0, 0, 0) == nwa * XCH


# ---- the dispatch table
def attn_kernel_for(mode, f16x2, bf16x3, C, heads, HW, wide_from, band_hw_max):
    if mode == 1 or heads <= 0 or C <= 0 or C % heads:
        return AK_NAIVE
    D = C // heads
    if D % 32 or HW <= 0 or HW % 32:
        return AK_NAIVE
    np_ = 2 if (mode == 3 or (mode == 0 and f16x2)) else 3 if (mode == 4 or (mode == 0 and bf16x3)) else 0
    if np_ and D <= AK_SPLIT_D_MAX:
        return AK_SPLIT2 if np_ == 2 else AK_SPLIT3
    band = D >= wide_from and (np_ == 2 or HW <= band_hw_max)              # 128 < D <= 256: the measured verdict
    if np_ and AK_WIDE_D_MIN <= D <= AK_WIDE_D_MAX and (D > AK_F32_D_MAX or band):
        return AK_WIDE2 if np_ == 2 else AK_WIDE3
    return AK_FLASH_F32 if D <= AK_F32_D_MAX else AK_NAIVE


def test_dispatch_table():
    src = _src("attn_kernels.h")
    for name, val in (("AK_NAIVE", 0), ("AK_FLASH_F32", 1), ("AK_SPLIT2", 2), ("AK_SPLIT3", 3), ("AK_SPLIT3_PRESPLIT", 4), ("AK_WIDE2", 5), ("AK_WIDE3", 6)):
        assert re.search(r"\b%s = %d\b" % (name, val), src), name
    assert _const(src, "AK_SPLIT_D_MAX") == AK_SPLIT_D_MAX and _const(src, "AK_F32_D_MAX") == AK_F32_D_MAX
    assert _const(src, "AK_WIDE_D_MIN") == AK_WIDE_D_MIN == D_MIN and _const(src, "AK_WIDE_D_MAX") == AK_WIDE_D_MAX == D_MAX
    wide_from = _const(src, "AK_WIDE_FROM_D")
    assert wide_from % 32 == 0 and 160 <= wide_from <= 288
    band_hw = _const(src, "AK_WIDE3_BAND_HW_MAX")
    assert band_hw % 32 == 0 and band_hw >= 64                               # the 8 x 8 cases of tests/test_gpu_attention_wide.py run the wide kernel

    def table(mode, f, b3, C, heads, HW):
        return attn_kernel_for(mode, f, b3, C, heads, HW, wide_from, band_hw)
    for line in ("if (mode == 1 || heads <= 0 || C <= 0 || C % heads != 0) return AK_NAIVE;",
                 "if (D % 32 != 0 || HW <= 0 || HW % 32 != 0) return AK_NAIVE;",
                 "const int np = (mode == 3 || (mode == 0 && f16x2)) ? 2 : (mode == 4 || (mode == 0 && bf16x3)) ? 3 : 0;",
                 "if (np && D <= AK_SPLIT_D_MAX) return np == 2 ? AK_SPLIT2 : AK_SPLIT3;",
                 "const bool band = D >= AK_WIDE_FROM_D && (np == 2 || HW <= AK_WIDE3_BAND_HW_MAX);",
                 "if (np && D >= AK_WIDE_D_MIN && D <= AK_WIDE_D_MAX && (D > AK_F32_D_MAX || band)) return np == 2 ? AK_WIDE2 : AK_WIDE3;",
                 "return D <= AK_F32_D_MAX ? AK_FLASH_F32 : AK_NAIVE;"):
        assert line in src, line
    assert "static_assert(table_sound()" in src
    # the launcher and the model go through the table, not through `if` chains of their own
    h2 = _src("kernels", "attention_h2.cpp")
    assert "attn_kernel_for(mode, f16x2, bf16x3, C, heads, HW)" in h2 and "attention_h2_supported(C, heads, HW);\n    if (sup" not in h2

    def before(mode, f, b3, D):            # launch_attention before the table existed
        if mode == 1:
            return AK_NAIVE
        if D <= 128 and (mode == 3 or (mode == 0 and f)):
            return AK_SPLIT2
        if D <= 128 and (mode == 4 or (mode == 0 and b3)):
            return AK_SPLIT3
        return AK_FLASH_F32 if D <= 256 else AK_NAIVE

    for D in range(32, 1024 + 1, 32):
        for mode in range(5):
            for f in (0, 1):
                for b3 in (0, 1):
                    np_ = 2 if (mode == 3 or (mode == 0 and f)) else 3 if (mode == 4 or (mode == 0 and b3)) else 0
                    wide = AK_WIDE2 if np_ == 2 else AK_WIDE3
                    for HW in (64, 256, 1024):
                        k = table(mode, f, b3, D, 1, HW)
                        assert k == table(mode, f, b3, 2 * D, 2, HW)                     # the head dim decides, not C
                        if D <= 128 or mode in (1, 2) or np_ == 0:
                            assert k == before(mode, f, b3, D), (D, mode, f, b3)        # today's rows and the comparison legs do not move
                        elif D > 256:
                            assert k == wide, (D, HW, mode, f, b3)
                        else:                                                            # 160 ... 256: the measured verdict
                            in_band = D >= wide_from and (np_ == 2 or HW <= band_hw)
                            assert k == (wide if in_band else AK_FLASH_F32), (D, HW, mode, f, b3)
                    # tokens or head dims that are no multiple of 32 stay on the one-thread-per-query kernel
                    assert table(mode, f, b3, D, 1, 16) == AK_NAIVE
                    assert table(mode, f, b3, D + 16, 1, 64) == AK_NAIVE
    assert table(0, 0, 1, 1056, 1, 64) == AK_NAIVE and table(4, 0, 0, 1024, 1, 64) == AK_WIDE3


def test_the_token_count_cases_expect_what_the_table_says():
    """tests/test_gpu_parity.py::test_attention_token_counts_with_a_ragged_last_query_tile spells out the kernel per case."""
    from tests import test_gpu_parity as P
    src = _src("attn_kernels.h")
    wide_from, band_hw = _const(src, "AK_WIDE_FROM_D"), _const(src, "AK_WIDE3_BAND_HW_MAX")
    seen = set()
    for D, mode, kern in P._TOKEN_COUNT_KERNELS:
        for S in (32, 96, 160, 288):
            must = kern[S] if isinstance(kern, dict) else kern
            assert must == attn_kernel_for(mode, 0, 1, 3 * D, 3, S, wide_from, band_hw), (D, mode, S)
            seen.add(must)
    assert seen == {AK_FLASH_F32, AK_SPLIT2, AK_SPLIT3, AK_WIDE2, AK_WIDE3}


def test_the_exports_are_declared():
    hdr = open(os.path.join(ROOT, "include", "mcvd_hip.h")).read()
    lib = open(os.path.join(ROOT, "mcvd_pytorch_amd", "_lib.py")).read()
    for name in ("mcvd_last_attention_kernel", "mcvd_model_op_attention_kernel"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert '"%s"' % name in lib, name
