"""CPU: the GroupNorm coefficient table of the Winograd 3x3 kernels with up to 2048 channels per sample on planes other than 8 x 8 -- the walk of
tests/test_wide_conv_cpu.py restated for the rule with two table sizes, its helpers imported.

The kernels (conv_wino3.cpp, conv_wino2h.cpp with two pieces or one: 512 threads; conv_wino.cpp: 1024 threads):
  * regions of 8 x 16 pixels (every plane but 8 x 8): ONE sample per workgroup, PC = CinP / max(P, 1) <= WINO_TABLE_CH_PLANE = 2048 entries; thread
    tid fetches entries tid + k * NT, k < 4 (conv_wino.cpp: k < 2), of channel min(16 c_begin + tid + k * NT, Cin - 1), and parks those below PC.
    Entries 2 and 3 (conv_wino.cpp: 1) are requested only where PC > 2 * NT (PC > NT), a condition uniform over the workgroup: a launch of
    PC <= 1024 issues what it always did.
  * G8 (8 x 8, two samples per workgroup): PC <= WINO_TABLE_CH = 1024, two entries per thread and sample (conv_wino.cpp: one) -- four for two
    samples do not fit the LDS (tests/test_wide_conv_cpu.py::test_the_whole_cin_table_would_not_fit).
  * the reader is unchanged: entry min((ch - c_begin) * 16 + cc, PC - 1) (+ img * PC).
  * the rule (conv_kernels.h: wino_admits; tests/wino_rule.py): Cin <= (P >= 4 ? WINO_MAX_CIN_K4 : WINO_MAX_CIN) and
    CinP / max(P, 1) <= (8 x 8 ? WINO_TABLE_CH : WINO_TABLE_CH_PLANE), next to the conditions of the split itself.

The 2-way split at 2304 channels: a part of 1152 channels fits a plane's table, but `Cin <= WINO_MAX_CIN` for splits of fewer than four parts is
part of the rule and stays (conv_kernels.h asserts the case; model.cpp sizes and offers by it), so (2304, P = 2) is
refused on every plane -- by the channel bound, no longer by the table.  test_the_rule_refuses_and_admits_what_it_must says so.
"""
import os
import re

import numpy as np

from tests import test_wide_conv_cpu as T
from tests import wino_rule

CK = T.CK
LDS_MAX = T.LDS_MAX
WINO_MAX_CIN = T.WINO_MAX_CIN
WINO_MAX_CIN_K4 = wino_rule.WINO_MAX_CIN_K4
WINO_TABLE_CH = T.WINO_TABLE_CH
WINO_TABLE_CH_PLANE = wino_rule.WINO_TABLE_CH_PLANE
# (threads, table entries per thread and sample: regions of a plane, G8, K parts the family has)
FAMILY_512 = dict(NT=512, NE=4, NE_G8=2, parts=(1, 2, 4, 8))          # conv_wino3.cpp; conv_wino2h.cpp: parts up to 4
FAMILY_1024 = dict(NT=1024, NE=2, NE_G8=1, parts=(1, 2))              # conv_wino.cpp


def table_ch(g8):
    return WINO_TABLE_CH if g8 else WINO_TABLE_CH_PLANE


def admitted(Cin, CinP, P, g8):
    """The bf16x3 family at 8 x 8 or on a 16 x 16 plane (the fp16 kernels: the same, 4 parts at most; conv_wino.cpp: 2 parts at most)."""
    return wino_rule.admits("WINO3", Cin, CinP, P, plane=8 if g8 else 16)


def admitted_parent(Cin, CinP, P):
    """The rule of the commit before: one table size (tests/test_w288_cpu.py)."""
    nch = CinP // CK
    return (Cin <= (WINO_MAX_CIN_K4 if P >= 4 else WINO_MAX_CIN) and CinP % CK == 0 and CinP // max(P, 1) <= WINO_TABLE_CH
            and (P < 2 or (P in (2, 4, 8) and nch % P == 0 and nch >= 2 * P)))


def check_tables(Cin, CinP, P, g8, fam):
    NT, NE = fam["NT"], fam["NE_G8"] if g8 else fam["NE"]
    nch = CinP // CK
    PC = CK * (nch // max(P, 1))
    assert PC == CinP // max(P, 1) and PC <= table_ch(g8) and PC <= NE * NT
    wide = (not g8) and PC > (NE // 2) * NT                               # the kernels' workgroup-uniform guard of the upper half of the entries
    ns = 2 if g8 else 1
    tid = np.arange(NT)
    covered = np.zeros(CinP, dtype=np.int64)
    for kh in range(max(P, 1)):
        c_begin, c_end = T.part_range(nch, max(P, 1), kh)
        assert 0 <= c_begin < c_end <= nch and c_end - c_begin >= (2 if P >= 2 else 1)
        table = np.full((ns * PC, 2), -1, dtype=np.int64)                 # (sample, channel) parked at each entry
        writes = np.zeros(ns * PC, dtype=np.int64)
        for k in range(NE):
            idx, src = tid + k * NT, np.minimum(CK * c_begin + tid + k * NT, Cin - 1)
            assert (src >= 0).all() and (src < Cin).all()                 # the global read stays inside coef[b][Cin]
            keep = idx < PC
            if not g8 and k >= NE // 2 and not wide:                      # not requested: nothing of it may be needed
                assert not keep.any(), (Cin, P, kh, k)
                continue
            for s in range(ns):
                assert (idx[keep] + s * PC < ns * PC).all()
                table[idx[keep] + s * PC, 0] = s
                table[idx[keep] + s * PC, 1] = src[keep]
                writes[idx[keep] + s * PC] += 1
        assert (writes == 1).all(), (Cin, P, kh)                           # every entry written exactly once
        lo, hi = CK * c_begin, min(CK * c_end, Cin)                        # the real channels this part's chunks read
        for s in range(ns):
            own = table[s * PC:s * PC + max(hi - lo, 0)]
            assert (own[:, 0] == s).all() and (own[:, 1] == np.arange(lo, hi)).all(), (Cin, P, kh)
            assert (table[s * PC + max(hi - lo, 0):(s + 1) * PC, 1] == Cin - 1).all()             # padding: the clamped source
        covered[lo:hi] += 1
        ch = np.repeat(np.arange(c_begin, c_end + 2), CK)                  # the reader, and the K loop's look-ahead past c_end
        cc = np.tile(np.arange(CK), c_end + 2 - c_begin)
        for img in range(ns):
            ri = T.reader_index(ch, cc, img, c_begin, PC)
            assert (ri >= 0).all() and (ri < ns * PC).all(), (Cin, P, kh)
            absolute = ch * CK + cc
            real = (ch < c_end) & (absolute < Cin)
            assert (table[ri[real], 1] == absolute[real]).all() and (table[ri[real], 0] == img).all(), (Cin, P, kh)
    assert (covered[:Cin] == 1).all() and (covered[Cin:] == 0).all()
    if NT == 512:
        for name, fn in (("wino3", T.lds_wino3), ("wino2h", T.lds_wino2h), ("wino1h", T.lds_wino1h)):
            if name == "wino3" or P in (1, 2, 4):
                assert fn(PC, g8) <= LDS_MAX, (name, Cin, P, g8, fn(PC, g8))
    else:
        assert T.lds_wino(PC, g8) <= LDS_MAX, (Cin, P, g8)


def test_every_admitted_layer_up_to_2304_channels_parks_and_reads_its_own_channels():
    cases = new = 0
    for CinP in range(CK, 2304 + 1, CK):
        for Cin in sorted({CinP, CinP - 7, CinP - 15}):
            for P in (1, 2, 4, 8):
                for g8 in (False, True):
                    ok = admitted(Cin, CinP, P, g8)
                    # nothing the parent admitted is lost, nothing moves at 8 x 8, and what is new is a plane with more than 1024 channels per part
                    assert ok or not admitted_parent(Cin, CinP, P), (Cin, CinP, P, g8)
                    if g8:
                        assert ok == admitted_parent(Cin, CinP, P), (Cin, CinP, P)
                    if not ok:
                        continue
                    if not admitted_parent(Cin, CinP, P):
                        assert not g8 and CinP // max(P, 1) > WINO_TABLE_CH and P in (1, 2), (Cin, CinP, P)
                        new += 1
                    check_tables(Cin, CinP, P, g8, FAMILY_512)
                    if P in FAMILY_1024["parts"]:
                        check_tables(Cin, CinP, P, g8, FAMILY_1024)
                    cases += 1
    print(f"{cases} admitted (Cin, CinP, parts, G8) table walks, {new} of them new")
    # unsplit, CinP 1040 .. 2048: 64 chunk counts x 3 Cin = 192; nothing new with a split (a 2-way part above 1024 channels needs Cin > 2048)
    assert new == 64 * 3, new


def test_the_rule_refuses_and_admits_what_it_must():
    assert not admitted(1040, 1040, 1, True) and admitted(1040, 1040, 1, False)
    assert admitted(1024, 1024, 1, True) and admitted(1024, 1024, 1, False)
    assert admitted(2048, 2048, 1, False) and admitted(2035, 2048, 1, False) and not admitted(2048, 2048, 1, True)
    assert not any(admitted(2064, 2064, 1, g8) for g8 in (False, True))
    assert not any(admitted(2049, 2064, 1, g8) for g8 in (False, True))
    assert not admitted(2304, 2304, 2, True)
    # a 2-way part of 1152 channels fits a plane's table; the launch stays refused by the channel bound of splits of fewer than four parts
    assert 2304 // 2 <= table_ch(False) and 2304 > WINO_MAX_CIN and not admitted(2304, 2304, 2, False)
    assert admitted(2304, 2304, 4, False) and admitted(2304, 2304, 4, True)
    # the two 32 x 32 up-path layers of the full ngf-288 net, and the 16 x 16 layers of the UCF-101 nets, unsplit
    for cin in (1440, 1152, 1344, 1728):
        assert admitted(cin, cin, 1, False) and not admitted_parent(cin, cin, 1)


def test_lds_requests_at_the_widest_plane_table():
    assert T.lds_wino3(2048, False) == 151616 <= LDS_MAX
    assert T.lds_wino2h(2048, False) == 124960 == T.lds_wino2h(1024, True)
    assert T.lds_wino1h(2048, False) == 92192 > LDS_MAX // 2             # one workgroup per CU at this width
    assert T.lds_wino(2048, False) == 112672 <= LDS_MAX
    assert T.lds_wino3(2048, True) > LDS_MAX                             # why 8 x 8 keeps the smaller table


def test_every_family_parks_by_the_two_table_sizes():
    assert wino_rule.header_constants()["WINO_TABLE_CH_PLANE"] == 2048 == 2 * WINO_TABLE_CH
    for fam in ("WINO3", "WINO2H", "WINO1H", "WINO"):
        assert wino_rule.admits(fam, 2048, plane=16) and wino_rule.admits(fam, 1040, plane=32) and not wino_rule.admits(fam, 2064, plane=16), fam
        assert wino_rule.admits(fam, 1024, plane=8) and not wino_rule.admits(fam, 1040, plane=8), fam
        assert wino_rule.admits(fam, 2048, parts=2, plane=8) and wino_rule.admits(fam, 2048, parts=2, plane=16), fam
    # conv_wino.cpp makes an unsplit launch of every ksplit but 2: its part is then all of CinP
    assert wino_rule.kernel_parts("WINO", 4) == 1 and not wino_rule.admits("WINO", 2048, parts=wino_rule.kernel_parts("WINO", 4), plane=8)
    assert wino_rule.admits("WINO", 1040, plane=16) and not wino_rule.admits("WINO", 1040, plane=16, spade=True)      # the SPADE-fused loader stays
    assert not wino_rule.admits("WINO3P", 1040, plane=16) and not wino_rule.admits("WINO3P", 1040, parts=2, plane=16)   # and so does the persistent kernel
    assert "WINO_TABLE_CH_PLANE" not in T._src(os.path.join("kernels", "conv_wino3p.cpp"))


def test_the_kernels_fill_the_table_as_restated():
    for f in ("conv_wino3.cpp", "conv_wino2h.cpp"):
        src = T._src(os.path.join("kernels", f))
        assert "constexpr int NE = G8 ? 2 : 4;" in src and "const bool wide = !G8 && PC > 2 * NT;" in src, f
        assert re.search(r"for \(int k = 0; k < NE; \+\+k\)\s*(//[^\n]*)?\n\s*if \(tid \+ k \* NT < PC\)", src), f
        assert "min(CK * c_begin + tid + k * NT, Cin - 1)" in src, f
    src = T._src(os.path.join("kernels", "conv_wino3.cpp"))
    assert re.search(r"if \(G8 \|\| wide\)\s*asm volatile\(\"global_load_dwordx2 v\[176:177\]", src)
    assert "static_assert(W3_PP != 24 || wino3_lds_bytes(WINO_TABLE_CH_PLANE, false) == 151616" in src
    src = T._src(os.path.join("kernels", "conv_wino2h.cpp"))
    assert re.search(r"if \(wide\)\s*asm volatile\(\"global_load_dwordx2 v\[220:221\]", src)
    assert "wino2h_lds_bytes(2, WINO_TABLE_CH_PLANE, false) == 124960 && wino2h_lds_bytes(1, WINO_TABLE_CH_PLANE, false) == 92192" in src
    src = T._src(os.path.join("kernels", "conv_wino.cpp"))
    assert "const bool wide = PRO && PRO != 3 && !G8 && PC > NT;" in src
    assert "min(CK * c_begin + tid + NT, Cin - 1)" in src and "if (wide && tid + NT < PC)" in src
    assert "wino_lds_bytes(WINO_TABLE_CH_PLANE, false) == 112672" in src
