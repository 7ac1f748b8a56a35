"""CPU: tests/wino_rule.py IS the admission rule of conv_kernels.h -- the rows compared number by number, every case the header static_asserts
evaluated with admits() -- and the expectations of tests/test_gpu_wino_admission.py follow from the rule and the fallback lists."""
import re

from tests import wino_rule as WR


def test_the_constants_and_rows_are_the_headers():
    c = WR.header_constants()
    assert c == dict(WINO_MAX_CIN=WR.WINO_MAX_CIN, WINO_MAX_CIN_K4=WR.WINO_MAX_CIN_K4, WINO_TABLE_CH=WR.WINO_TABLE_CH,
                     WINO_TABLE_CH_PLANE=WR.WINO_TABLE_CH_PLANE), c
    rows = WR.header_rules()
    assert rows == WR.RULES, rows
    src = open(WR.HEADER).read()
    assert "r.family == (f == CF_WINO1H ? CF_WINO2H : f)" in src                                   # the one-piece family reads the two-piece row
    assert "return f == CF_WINO ? (ksplit == 2 ? 2 : 1) : ksplit;" in src                           # kernel_parts
    assert "return parts >= 4 ? WINO_MAX_CIN_K4 : WINO_MAX_CIN;" in src and "return g8 ? WINO_TABLE_CH : WINO_TABLE_CH_PLANE;" in src


def test_every_case_the_header_asserts_evaluates_the_same_here():
    cases = WR.header_cases()
    src = open(WR.HEADER).read()
    body = src[src.index("kWinoCases[] = {"):src.index("constexpr WinoLaunch wino_case_launch")]
    assert len(cases) == body.count("{CF_") >= 60, (len(cases), body.count("{CF_"))                # every row parsed
    assert "static_assert(first_wrong_wino_case() == -1" in src
    for fam, Cin, CinP, ksplit, plane, C0, spade, want in cases:
        got = WR.admits(fam, Cin, CinP, WR.kernel_parts(fam, ksplit), plane, C0=C0 or None, spade=spade)
        assert got == want, (fam, Cin, CinP, ksplit, plane, C0, spade, want)
    have = {c[:5] + (c[7],) for c in cases}
    for must in (("WINO3P", 1040, 1040, 0, 16, False), ("WINO3P", 1040, 1040, 2, 16, False), ("WINO3P", 48, 48, 0, 16, False),
                 ("WINO3P", 96, 96, 2, 16, False), ("WINO3P", 96, 96, 0, 16, True), ("WINO", 48, 48, 4, 8, True),
                 ("WINO2H", 1088, 1088, 4, 8, True), ("WINO2H", 1040, 1040, 4, 8, False), ("WINO2H", 2320, 2320, 4, 8, False),
                 ("WINO3", 2304, 2304, 2, 16, False), ("WINO3", 2304, 2304, 4, 8, True), ("WINO3", 2304, 2304, 8, 8, True)):
        assert must in have, must
    assert ("WINO", 1152, 1152, 0, 16, 0, True, False) in cases and ("WINO", 1152, 1152, 0, 16, 0, False, True) in cases


def test_every_plane_case_the_header_asserts_evaluates_the_same_here():
    """The geometric clause -- H % 8, W % 16, the 8 x 8 pairs, max_hw -- over planes that are not square (kWinoPlaneCases)."""
    cases = WR.header_plane_cases()
    src = open(WR.HEADER).read()
    body = src[src.index("kWinoPlaneCases[] = {"):src.index("constexpr WinoLaunch wino_plane_case_launch")]
    assert len(cases) == body.count("{CF_") >= 20, (len(cases), body.count("{CF_"))                # every row parsed
    assert "static_assert(first_wrong_wino_plane_case() == -1" in src
    for fam, H, W, parts, Cin, want in cases:
        assert WR.admits(fam, Cin, Cin, parts, (H, W)) == want, (fam, H, W, parts, Cin, want)
    have = {c[:4] + (c[5],) for c in cases}
    for must in (("WINO3", 8, 16, 1, True), ("WINO3", 16, 8, 1, False), ("WINO3", 24, 16, 1, True), ("WINO3", 12, 16, 1, False),
                 ("WINO3", 128, 128, 1, True), ("WINO3", 128, 256, 1, False), ("WINO", 128, 256, 1, True), ("WINO3", 8, 16, 2, True)):
        assert must in have, must
    for fam in ("WINO", "WINO2H", "WINO1H", "WINO3", "WINO3P"):
        assert (fam, 8, 8, 1, fam != "WINO3P") in have, fam
    assert {c[5] for c in cases} == {True, False} and any(c[1] > c[2] for c in cases) and any(c[1] & (c[1] - 1) for c in cases if c[5])


def test_room_for_the_parts_and_missing_weights():
    assert WR.admits("WINO3", 1056, parts=2, part_floats=2 * 2 * 32 * 64) and not WR.admits("WINO3", 1056, parts=2, part_floats=2 * 2 * 32 * 64 - 1)
    assert not WR.admits("WINO3", 1056, parts=2, part_floats=0) and WR.admits("WINO3", 512, parts=1, part_floats=0)
    assert not WR.admits("WINO3", 512, weights=False) and not WR.admits("WINO3", 512, ks=1)
    assert not WR.admits("WINO3", 512, plane=(8, 24)) and WR.admits("WINO3", 512, plane=(8, 16)) and not WR.admits("WINO3", 512, plane=(12, 16))
    assert WR.admits("WINO", 64, plane=256, B=1) and not WR.admits("WINO3", 64, plane=256, B=1)                 # H * W <= 16384 but for conv_wino.cpp
    assert not WR.admits("WINO3", 512, plane=32, B=1024) and WR.admits("WINO3", 512, plane=32, B=1023)          # 2^29 patch offsets
    big = dict(plane=128, B=256, Cout=1 << 18)                                                                  # 2^31 items of the persistent kernel
    assert not WR.admits("WINO3P", 64, **big) and WR.admits("WINO3", 64, **big) and WR.admits("WINO3P", 64, plane=128, B=256, Cout=1 << 17)


def _kernel_table():
    """{id: (family, kparts, weights, fallback ids)} parsed from kConvKernels."""
    src = open(WR.HEADER).read()
    enum = dict((n, int(v)) for n, v in re.findall(r"\b(CK_\w+) = (-?\d+)", src))
    body = src[src.index("kConvKernels[] = {"):src.index("kNoConvKernel")]
    rows = {}
    for name, fam, kp, wt, fb in re.findall(r"\{(CK_\w+),\s*\"\w+\",\s*CF_(\w+),\s*\d+,\s*\d+,\s*(\d+),\s*\w+,\s*(CW_\w+),[^{]*\{([^}]*)\}", body):
        rows[enum[name]] = (fam, int(kp), wt, [enum[t.strip()] for t in fb.split(",") if t.strip() != "-1"])
    return rows


def test_the_gpu_cases_follow_from_the_rule_and_the_fallback_lists():
    from tests import test_gpu_wino_admission as G
    table = _kernel_table()
    assert table[20][3] == [20, 17, 16, 11, 10, 4] and table[4] == ("WINO", 0, "CW_WPW", [4])
    assert len(G.CASES) == 18
    forced_families = set()
    for forced, C0, C1, H, runs in G.CASES:
        fam0, kp0, wt0, fallback = table[forced]
        forced_families.add(fam0)
        room = kp0 * G.B * G.COUT * H * H                      # mcvd_op_conv2d: scratch for the parts of the forced id
        ran = G.TILE
        for kid in fallback:
            fam, kp, wt, _ = table[kid]
            if WR.admits(fam, C0 + C1, -(-(C0 + C1) // 16) * 16, WR.kernel_parts(fam, kp), H, C0=C0, B=G.B, Cout=G.COUT,
                         weights=wt in (wt0, "CW_WPW"), part_floats=room):          # (id 4 is handed no K split by the stand-alone conv)
                ran = kid
                break
        assert ran == runs, (forced, C0, C1, H, runs, ran)
    assert forced_families == {"WINO", "WINO2H", "WINO1H", "WINO3", "WINO3P"}
