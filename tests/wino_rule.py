"""The admission rule of the Winograd 3x3 families (mcvd_pytorch_amd/csrc/conv_kernels.h: kWinoRules / wino_admits), restated once for the
tests.  tests/test_wino_rule_cpu.py compares the rows below with the header's and evaluates every case the header static_asserts (kWinoCases,
and kWinoPlaneCases for the planes that are not square) with admits(); tests/conv_ref.py asks it which id a forced launch ends in; the CPU walks (test_wide_conv_cpu, test_w288_cpu, test_wide_plane_cpu, test_f16_ksplit4_cpu) ask admits() what a launch takes.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "mcvd_pytorch_amd", "csrc", "conv_kernels.h")

WINO_MAX_CIN = 2048
WINO_MAX_CIN_K4 = 2304
WINO_TABLE_CH = 1024
WINO_TABLE_CH_PLANE = 2048

# family -> (chunk, serves 8 x 8 pairs, H * W cap or 0, fewest chunks per part unsplit / 2 / 4 / 8 parts (0: no such split), SPADE loader, persistent)
RULES = {
    "WINO":   (16, True, 0, (1, 2, 0, 0), True, False),
    "WINO2H": (16, True, 16384, (1, 2, 3, 0), False, False),
    "WINO3":  (16, True, 16384, (1, 2, 2, 2), False, False),
    "WINO3P": (16, False, 16384, (4, 4, 4, 4), False, True),
}


def kernel_parts(family, ksplit):
    """The K parts a kernel makes of ConvArgs::ksplit: conv_wino.cpp counts 2 as a split and every other value as none."""
    return (2 if ksplit == 2 else 1) if family == "WINO" else ksplit


def admits(family, Cin, CinP=None, parts=1, plane=8, C0=None, B=2, Cout=32, CoutP=None, ks=3, weights=True, spade=False, part_floats=None):
    """wino_admits.  plane: H = W, or (H, W).  C0: channels of the first source (default: one source).  part_floats: room for the partial
    results (default: exactly what the parts need -- the caller's buffer is not what the walks are about)."""
    chunk, g8_ok, max_hw, min_chunks, spade_ok, persistent = RULES["WINO2H" if family == "WINO1H" else family]
    H, W = plane if isinstance(plane, tuple) else (plane, plane)
    CinP = Cin if CinP is None else CinP
    C0 = Cin if C0 is None else C0
    C1 = Cin - C0
    CoutP = Cout if CoutP is None else CoutP
    if ks != 3 or not weights:
        return False
    g8 = H == 8 and W == 8
    if not ((H % 8 == 0 and W % 16 == 0 and H >= 8 and W >= 16) or (g8_ok and g8)):
        return False
    if max_hw and H * W > max_hw:
        return False
    if CinP % chunk != 0 or (C1 != 0 and C0 % chunk != 0):
        return False
    if B * max(C0, C1) * H * W >= 1 << 29:
        return False
    if spade and not (spade_ok and Cin <= WINO_TABLE_CH):
        return False
    parts = parts if parts >= 2 else 1
    slot = {1: 0, 2: 1, 4: 2, 8: 3}.get(parts, -1)
    if slot < 0 or min_chunks[slot] == 0:
        return False
    nch = CinP // chunk
    if nch % parts != 0 or nch // parts < min_chunks[slot]:
        return False
    if persistent:
        if Cin > WINO_TABLE_CH or B * (H // 8) * (W // 16) * (CoutP // 32) * 8 >= 1 << 31:
            return False
    elif Cin > (WINO_MAX_CIN_K4 if parts >= 4 else WINO_MAX_CIN) or CinP // parts > (WINO_TABLE_CH if g8 else WINO_TABLE_CH_PLANE):
        return False
    need = parts * B * Cout * H * W
    room = need if part_floats is None else part_floats
    return parts == 1 or (room != 0 and need <= room)


def header_constants():
    src = open(HEADER).read()
    return {n: int(v) for n, v in re.findall(r"constexpr int (WINO_\w+) = (\d+);", src)}


def header_rules():
    """{family: row} parsed from kWinoRules."""
    src = open(HEADER).read()
    body = src[src.index("kWinoRules[] = {"):src.index("constexpr const WinoRule* wino_rule")]
    rows = {}
    for fam, chunk, g8, hw, mc, sp, per in re.findall(r"\{CF_(\w+),\s*(\d+),\s*(true|false),\s*(\d+),\s*\{([\d, ]+)\},\s*(true|false),\s*(true|false)\}", body):
        rows[fam] = (int(chunk), g8 == "true", int(hw), tuple(int(v) for v in mc.split(",")), sp == "true", per == "true")
    return rows


def header_plane_cases():
    """[(family, H, W, parts, Cin, admitted)] parsed from kWinoPlaneCases, the header's static_asserted list of planes that are not square."""
    src = open(HEADER).read()
    body = src[src.index("kWinoPlaneCases[] = {"):src.index("constexpr WinoLaunch wino_plane_case_launch")]
    return [(fam, int(h), int(w), int(parts), int(cin), ad == "true")
            for fam, h, w, parts, cin, ad in re.findall(r"\{CF_(\w+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(true|false)\}", body)]


def header_cases():
    """[(family, Cin, CinP, ksplit, plane, C0, spade, admitted)] parsed from kWinoCases, the list the header static_asserts."""
    src = open(HEADER).read()
    body = src[src.index("kWinoCases[] = {"):src.index("constexpr WinoLaunch wino_case_launch")]
    return [(fam, int(cin), int(cinp), int(ks), int(pl), int(c0), sp == "true", ad == "true")
            for fam, cin, cinp, ks, pl, c0, sp, ad in
            re.findall(r"\{CF_(\w+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(true|false),\s*(true|false)\}", body)]
