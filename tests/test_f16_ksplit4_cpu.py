"""CPU: the 4-way K split of the two fp16 Winograd kernels (shape ids 26 / 27; conv_wino2h.cpp with two pieces and with one) -- the partition of the
16-channel chunks into parts, walked over every layer shape the rule admits (CinP up to 2304 channels).

The kernels: `nch = CinP / 16` chunks; workgroup (.., blockIdx.y = part) contracts chunks [part * nch / 4, (part + 1) * nch / 4) and writes its raw
partial result to a.part[part]; chunk c reads channels 16 c .. 16 c + 15 from x0 when 16 c < C0, else from x1 (one source per chunk).
The rule (conv_kernels.h: wino_admits, restated by tests/wino_rule.py): nch % 4 == 0, nch / 4 >= MINCH_K4 = 3 (the prologue requests the patches
of three chunks; a shorter part would fetch its neighbour's), no chunk across the concat seam (C1 == 0 or C0 % 16 == 0), Cin <= WINO_MAX_CIN_K4
= 2304 and a part of at most 1024 channels at 8 x 8 -- and room for four partial results, which is the caller's buffer and not walked here.  The
table rows and static_asserts of conv_kernels.h are checked by every build of the library.
"""
import os
import re

from tests import wino_rule

CK = 16
MINCH_K4 = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcvd_pytorch_amd", "csrc")


def usable_k4(Cin, CinP, C0, C1, plane=8):
    assert C0 + C1 == Cin
    ok = wino_rule.admits("WINO2H", Cin, CinP, 4, plane=plane, C0=C0)
    assert ok == wino_rule.admits("WINO1H", Cin, CinP, 4, plane=plane, C0=C0)          # one rule for both piece counts
    return ok


def parts(nch, ksp):
    """[(c_begin, c_end)] per blockIdx.y, the kernels' expression."""
    return [(kh * (nch // ksp), kh * (nch // ksp) + nch // ksp) for kh in range(ksp)]


def chunk_source(c, Cin, C0):
    """The source the loader picks for chunk c (LOAD_PR: cb = min(c * CK, Cin - 1); second = cb >= C0)."""
    return 1 if min(c * CK, Cin - 1) >= C0 else 0


def test_the_restated_minimum_is_the_kernels():
    f, name = "conv_wino2h.cpp", "H2_MINCH_K4"               # one kernel source, one constant, one row of the rule for both piece counts
    src = open(os.path.join(CSRC, "kernels", f)).read()
    m = re.findall(r"constexpr int \w*MINCH_K4 = (\d+);", src)
    assert m == [str(MINCH_K4)] and re.search(r"constexpr int %s = (\d+);" % name, src), (f, m)
    assert "wino_rule(CF_WINO2H)->min_chunks[2] == %s" % name in src, f"{f}: the rule's minimum is not pinned to the kernel's"
    assert wino_rule.RULES["WINO2H"][3][2] == MINCH_K4 and "WINO1H" not in wino_rule.RULES
    table = open(os.path.join(CSRC, "conv_kernels.h")).read()
    assert "CK_WINO2H_K4 = 26" in table and "CK_WINO1H_K4 = 27" in table


def test_every_admitted_layer_is_partitioned_soundly():
    admitted = wide = seam_inside_a_part = 0
    for CinP in range(CK, 2304 + CK + 1, CK):
        for Cin in sorted({CinP, CinP - 7, CinP - CK + 1}):         # full last chunk, padded ones
            # up to 1024 channels every seam; above, where nothing but the count changes, the seams on and next to the chunk boundaries
            seams = range(1, Cin + 1) if CinP <= 1024 else sorted({Cin} | {c + d for c in range(CK, Cin, CK) for d in (-1, 0, 1)})
            for C0 in seams:
                C1 = Cin - C0
                if not usable_k4(Cin, CinP, C0, C1):
                    assert CinP <= 2304 or Cin > 2304
                    continue
                admitted += 1
                wide += CinP > 1024
                nch = CinP // CK
                assert Cin <= 2304 and CinP // 4 <= 1024
                pp = parts(nch, 4)
                owner = [0] * nch
                for b, e in pp:
                    assert e - b >= MINCH_K4, (CinP, b, e)
                    assert 0 <= b < e <= nch
                    for c in range(b, e):
                        owner[c] += 1
                    # the three patches the prologue requests are this part's own chunks
                    assert b + 2 < e
                assert owner == [1] * nch, (CinP, pp)
                for c in range(nch):                                  # every channel of a chunk comes from the source the loader picks
                    lo, hi = c * CK, min(c * CK + CK, Cin)
                    if lo >= Cin:
                        continue
                    src = chunk_source(c, Cin, C0)
                    assert all((ch >= C0) == bool(src) for ch in (lo, hi - 1)), (Cin, C0, c)
                if C1 and any(b * CK < C0 < e * CK for b, e in pp):
                    seam_inside_a_part += 1
    print(f"{admitted} admitted (Cin, CinP, C0) layers, {wide} of them above 1024 channels; the seam inside a part {seam_inside_a_part} times")
    assert admitted > 1000 and wide > 1000 and seam_inside_a_part > 100, (admitted, wide, seam_inside_a_part)


def test_the_rule_refuses_what_it_must():
    assert usable_k4(192, 192, 192, 0)                      # 12 chunks: the shortest admissible parts
    assert not usable_k4(128, 128, 128, 0)                  # 8 chunks: parts of two, shorter than the prologue's three requests
    assert not usable_k4(288, 288, 288, 0)                  # 18 chunks: not divisible by 4
    assert not usable_k4(256, 256, 100, 156)                # the seam inside a chunk
    assert usable_k4(256, 256, 160, 96)                     # the seam inside a part (chunk 10 of 16), on a chunk boundary
    assert usable_k4(1088, 1088, 1088, 0)                   # 68 chunks, 272 channels per part: beyond the unsplit 8 x 8 table, inside a part's
    assert not usable_k4(1040, 1040, 1040, 0)               # 65 chunks do not divide by 4
    assert not usable_k4(2320, 2320, 2320, 0)               # 145 chunks, and above WINO_MAX_CIN_K4: the channel bound
    assert usable_k4(2304, 2304, 2304, 0) and not usable_k4(2368, 2368, 2368, 0)          # 148 chunks divide by 4: the channel bound alone
    assert usable_k4(250, 256, 250, 0)                      # a padded last chunk
    for plane in (8, 16):
        assert usable_k4(2304, 2304, 1152, 1152, plane) and not wino_rule.admits("WINO2H", 2304, parts=8, plane=plane)
