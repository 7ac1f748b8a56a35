"""CPU: the per-part GroupNorm coefficient table of the Winograd 3x3 kernels (conv_wino3.cpp, conv_wino2h.cpp with two pieces or one; conv_wino.cpp
with one entry per thread) and the rule that admits a layer, restated here and walked over every layer shape up to 2048 channels.

The kernels: `nch = CinP / 16` chunks; workgroup (.., blockIdx.y = kh) of a P-way K split contracts chunks [kh * nch / P, (kh + 1) * nch / P) and
parks the (A_c, B_c) pairs of THOSE channels only: PC = 16 * (nch / P) entries per sample (G8, two 8 x 8 images per workgroup: 2 * PC, the
second sample at offset PC).
  * source:  thread tid fetches entries tid and tid + 512 of channel min(16 * c_begin + tid + k * 512, Cin - 1) -- the clamp covers the padded
    last chunk of the last part -- and parks entry tid + k * 512 when it is below PC;
  * reader:  patch slot (chunk ch, channel code cc, image img) reads entry min((ch - c_begin) * 16 + cc, PC - 1) + img * PC; the clamp keeps the
    look-ahead of the K loop (it activates a patch of chunk c_end that nobody reads) inside the table;
  * the rule (conv_kernels.h: wino_admits; tests/wino_rule.py restates it): at 8 x 8, where this walk asks, Cin <= WINO_MAX_CIN = 2048 and
    CinP / max(P, 1) <= WINO_TABLE_CH = 1024 (two entries per thread and sample), next to the conditions of the split itself (nch % P == 0,
    at least two chunks per part; three for the 4-way split of the fp16 kernels: tests/test_f16_ksplit4_cpu.py) and room for the partial
    results, which is the caller's buffer and not walked here.
"""
import os
import re

import numpy as np

from tests import wino_rule

CK = 16
NT = 512
LDS_MAX = 160 * 1024
WINO_MAX_CIN = wino_rule.WINO_MAX_CIN
WINO_TABLE_CH = wino_rule.WINO_TABLE_CH
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcvd_pytorch_amd", "csrc")


def admitted(Cin, CinP, P):
    """The bf16x3 family at 8 x 8: one table of WINO_TABLE_CH entries per sample."""
    return wino_rule.admits("WINO3", Cin, CinP, P, plane=8)


def part_range(nch, P, kh):
    """[c_begin, c_end) of blockIdx.y = kh, the kernels' expression."""
    return kh * (nch // P), kh * (nch // P) + nch // P


def table_source(c_begin, tid, k, Cin):
    return np.minimum(CK * c_begin + tid + k * NT, Cin - 1)


def table_index(tid, k):
    return tid + k * NT


def reader_index(ch, cc, img, c_begin, PC):
    return np.minimum((ch - c_begin) * CK + cc, PC - 1) + img * PC


def chunk_source(c, Cin, C0):
    """The source the loader picks for chunk c (LOAD_PR: cb = min(c * CK, Cin - 1); second = cb >= C0)."""
    return 1 if min(c * CK, Cin - 1) >= C0 else 0


# the kernels' *_lds_bytes(pc, g8), pc = the part's channel count
def lds_wino3(pc, g8):
    vw = 3 * 16 * 2 * 4 * 32
    return (2 * vw + 2 * (CK * 10 * 24 + 8) + (4 if g8 else 2) * pc + (1 if g8 else 3) * NT) * 4


def lds_wino2h(pc, g8):          # wino2h_lds_bytes(2, pc, g8)
    vw = 2 * 16 * 2 * 4 * 32
    return (2 * vw + 2 * (CK * 10 * 24 + 4) + (4 if g8 else 2) * pc + 6 * NT) * 4


def lds_wino1h(pc, g8):          # wino2h_lds_bytes(1, pc, g8): the one-piece instantiations of conv_wino2h.cpp, one V plane
    vw = 16 * 2 * 4 * 32
    return (2 * vw + 2 * (CK * 10 * 24 + 4) + (4 if g8 else 2) * pc + 6 * NT) * 4


def lds_wino(pc, g8):
    return max((2 * CK * 16 * 32 + 2 * (CK * 10 * 24 + 4) + (4 if g8 else 2) * pc) * 4, 16 * 32 * 32 * 4)


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_kernels_write_the_expressions_restated_here():
    """(The rule itself is not read off the sources: tests/test_wino_rule_cpu.py compares tests/wino_rule.py with the header's table and cases.)"""
    assert re.search(r"constexpr int wino_part_channels\(int CinP, int parts\) \{ return CinP / \(parts >= 2 \? parts : 1\); \}", _src("conv_kernels.h"))
    for f in ("conv_wino3.cpp", "conv_wino2h.cpp", "conv_wino.cpp"):
        src = _src(os.path.join("kernels", f))
        assert not re.search(r"a\.Cin <= 1024", src), f"{f}: a bare 1024"
        assert "lds_bytes(a.Cin" not in src, f"{f}: the LDS size still takes all Cin channels"
    for f in ("conv_wino3.cpp", "conv_wino2h.cpp"):        # the expressions restated above, as the kernels write them
        src = _src(os.path.join("kernels", f))
        assert "min(CK * c_begin + tid + k * NT, Cin - 1)" in src, f
        assert re.search(r"min\(\(\(ch\) - c_begin\) \* CK \+ \(int\)\(\(p_pk\[sl\] >> 12\) & \(CK - 1\)\), PC - 1\) \+ "
                         r"\(G8 \? \(int\)\(\(p_pk\[sl\] >> 20\) & 1u\) \* PC : 0\)", src), f
        assert "const int PC = (nch_all / ksp) * CK;" in src and "if (tid + k * NT < PC)" in src, f
    # the fp16 kernel serves two piece counts: its V-plane word count, and with it the LDS request (lds_wino2h / lds_wino1h above), carries NP
    src = _src(os.path.join("kernels", "conv_wino2h.cpp"))
    assert "constexpr int h2_vw(int np) { return np * 16 * 2 * 4 * H2_T; }" in src and "VW = h2_vw(NP);" in src
    assert "return (size_t)(2 * h2_vw(np) + 2 * (H2_CK * 10 * H2_PP + 4) + (g8 ? 4 : 2) * pc + 6 * H2_NT) * sizeof(float);" in src
    assert "const size_t lds = wino2h_lds_bytes(NP, wino_part_channels(a.CinP, a.ksplit), G8);" in src
    src = _src(os.path.join("kernels", "conv_wino.cpp"))
    assert "min(CK * c_begin + tid, Cin - 1)" in src and "const int PC = (nch_all / ksp) * CK;" in src
    assert "min(((ch) - c_begin) * CK + (p_ci[sl] & (CK - 1)), PC - 1) + (G8 ? p_img[sl] * PC : 0)" in src
    # the persistent kernel keeps whole-Cin tables: its LDS request takes Cin, and the rule holds Cin itself to the table
    assert "wino3p_lds_bytes(a.Cin)" in _src(os.path.join("kernels", "conv_wino3p.cpp"))
    assert not wino_rule.admits("WINO3P", 1040, plane=16) and not wino_rule.admits("WINO3P", 1040, parts=2, plane=16) and wino_rule.admits("WINO3P", 1024, plane=16)


def _check_tables(Cin, CinP, P, g8):
    nch = CinP // CK
    PC = CK * (nch // max(P, 1))
    assert PC == CinP // max(P, 1) and PC <= WINO_TABLE_CH
    ns = 2 if g8 else 1
    tid = np.arange(NT)
    covered = np.zeros(CinP, dtype=np.int64)
    for kh in range(max(P, 1)):
        c_begin, c_end = part_range(nch, max(P, 1), kh)
        assert 0 <= c_begin < c_end <= nch and c_end - c_begin >= (2 if P >= 2 else 1)
        table = np.full((ns * PC, 2), -1, dtype=np.int64)             # (sample, channel) parked at each entry
        writes = np.zeros(ns * PC, dtype=np.int64)
        for k in range(2):
            idx, src = table_index(tid, k), table_source(c_begin, tid, k, Cin)
            assert (src >= 0).all() and (src < Cin).all()             # the global read stays inside coef[b][Cin]
            keep = idx < PC
            for s in range(ns):
                assert (idx[keep] + s * PC < ns * PC).all()
                table[idx[keep] + s * PC, 0] = s
                table[idx[keep] + s * PC, 1] = src[keep]
                writes[idx[keep] + s * PC] += 1
        assert (writes == 1).all(), (Cin, P, kh)                       # two entries per thread and sample fill the table, each once
        lo, hi = CK * c_begin, min(CK * c_end, Cin)                    # the real channels this part's chunks read
        for s in range(ns):
            own = table[s * PC:s * PC + max(hi - lo, 0)]
            assert (own[:, 0] == s).all() and (own[:, 1] == np.arange(lo, hi)).all(), (Cin, P, kh)        # each parked once, at its place
            assert (table[s * PC + max(hi - lo, 0):(s + 1) * PC, 1] == Cin - 1).all()                    # padding: the clamped source
        covered[lo:hi] += 1
        # the reader: every (chunk, channel code, image) of the part, and the K loop's look-ahead past c_end
        ch = np.repeat(np.arange(c_begin, c_end + 2), CK)
        cc = np.tile(np.arange(CK), c_end + 2 - c_begin)
        for img in range(ns):
            ri = reader_index(ch, cc, img, c_begin, PC)
            assert (ri >= 0).all() and (ri < ns * PC).all(), (Cin, P, kh)
            absolute = ch * CK + cc
            real = (ch < c_end) & (absolute < Cin)
            assert (table[ri[real], 1] == absolute[real]).all() and (table[ri[real], 0] == img).all(), (Cin, P, kh)
    assert (covered[:Cin] == 1).all() and (covered[Cin:] == 0).all()
    for name, fn in (("wino3", lds_wino3), ("wino2h", lds_wino2h), ("wino1h", lds_wino1h)):
        if name == "wino3" or P in (1, 2, 4):
            assert fn(PC, g8) <= LDS_MAX, (name, Cin, P, g8, fn(PC, g8))
    if P in (1, 2):
        assert lds_wino(PC, g8) <= LDS_MAX


def test_every_admitted_layer_parks_and_reads_its_own_channels():
    cases = wide = seam_inside_a_part = 0
    for CinP in range(CK, 2048 + 1, CK):
        for Cin in sorted({CinP, CinP - 7, CinP - 15}):
            for P in (1, 2, 4, 8):
                if not admitted(Cin, CinP, P):
                    assert Cin > 1024 or P >= 2, (Cin, P)            # every layer up to 1024 channels is still admitted unsplit
                    continue
                for g8 in (False, True):
                    _check_tables(Cin, CinP, P, g8)
                    cases += 1
                nch = CinP // CK
                pp = [part_range(nch, P, kh) for kh in range(P)]
                # the concat: C1 == 0, or a seam on a chunk boundary (C0 % 16 == 0: a chunk never straddles it).  The table does not know the
                # seam; the loader picks one source per chunk
                lo = np.arange(nch) * CK
                lo = lo[lo < Cin]
                last = np.minimum(lo + CK, Cin) - 1
                for C0 in [Cin] + list(range(CK, Cin, CK)):
                    src = np.array([chunk_source(int(c), Cin, C0) for c in lo // CK], dtype=bool)
                    assert ((lo >= C0) == src).all() and ((last >= C0) == src).all(), (Cin, C0)
                    if Cin > 1024:
                        wide += 1
                        if C0 < Cin and any(b * CK < C0 < e * CK for b, e in pp):
                            seam_inside_a_part += 1
    print(f"{cases} admitted (Cin, CinP, parts, G8) table walks; {wide} admitted (Cin, CinP, parts, C0) layers above 1024 channels, "
          f"{seam_inside_a_part} of them with the concat seam inside a part")
    assert wide >= 1000 and seam_inside_a_part > 100, (cases, wide, seam_inside_a_part)


def test_the_whole_cin_table_would_not_fit():
    """What the per-part table replaces: [G8: 2][Cin] entries at Cin = 2048 are 64 bytes more LDS than a CU has."""
    assert lds_wino3(2048, True) == LDS_MAX + 64
    assert lds_wino3(1024, True) < lds_wino3(2048, True) and lds_wino3(1024, True) <= LDS_MAX


def test_the_rule_refuses_what_it_must():
    assert not admitted(1040, 1040, 1)                      # unsplit launches stay at 1024
    assert admitted(1024, 1024, 1) and admitted(1017, 1024, 1)
    assert not any(admitted(2064, 2064, P) for P in (1, 2, 4, 8))
    assert not any(admitted(2049, 2064, P) for P in (1, 2, 4, 8))
    assert admitted(1536, 1536, 2) and admitted(1536, 1536, 4) and admitted(1536, 1536, 8)
    assert admitted(2048, 2048, 2) and admitted(2048, 2048, 8)
    assert not admitted(2048, 2048, 1)
    assert admitted(1050, 1056, 2)                          # a padded last chunk in the last part
    assert not admitted(1050, 1056, 4)                      # 66 chunks do not divide by 4
    assert admitted(1344, 1344, 2) and admitted(1344, 1344, 4) and not admitted(1344, 1344, 8)          # 84 chunks
    assert admitted(1152, 1152, 8)
