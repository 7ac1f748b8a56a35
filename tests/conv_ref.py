"""The stand-alone conv (mcvd_op_conv2d) restated in float64, the inputs its tests run on and the kernel id a forced launch must take (plain
torch on the CPU; nothing here touches the GPU or the library).  A helper of tests/test_gpu_conv_paths.py, tests/test_conv_paths_cpu.py
and tools/conv_paths_accuracy.py.

A case names one launch: the forced shape id, the kernel size, the batch, the channels of the two sources of the virtual concat, the
output channels, the plane, the loader path (`coef`: the GroupNorm affine A x + B; `act`: SiLU behind it), the residual (with it the
1/sqrt(2) scale of the ResBlocks), the data kind and the options `conv_cot` / `persist_grid`.

What must run (expected_id) comes from the fallback lists of conv_kernels.h, tests/wino_rule.admits and a restatement of the two 1x1
predicates (conv1x1_h2_supported, conv1x1_dma_supported) -- never from the library's own answer.
"""
import collections
import functools
import os
import re

import torch
import torch.nn.functional as F

from tests import wino_rule as WR

F64 = torch.float64
RES_SCALE = 0.70710678

Case = collections.namedtuple("Case", "kid ks B C0 C1 Cout H W coef act res kind cot pgrid stats")


def case(kid, ks, B, C0, C1, Cout, plane, coef=True, act=1, res=False, kind="gauss", cot=0, pgrid=0, stats=False):
    H, W = plane if isinstance(plane, tuple) else (plane, plane)
    return Case(kid, ks, B, C0, C1, Cout, H, W, bool(coef), int(act), bool(res), kind, cot, pgrid, bool(stats))


def case_id(c):
    pro = ("silu" if c.act else "affine") if c.coef else "raw"
    return (f"id{c.kid}_k{c.ks}_B{c.B}_c{c.C0}+{c.C1}_o{c.Cout}_{c.H}x{c.W}_{pro}" + ("_res" if c.res else "") + f"_{c.kind}"
            + (f"_cot{c.cot}" if c.cot else "") + (f"_g{c.pgrid}" if c.pgrid else "") + ("_stats" if c.stats else ""))


def data_key(c):
    """What the inputs and the reference depend on: everything but the kernel and its options."""
    return c._replace(kid=-1, cot=0, pgrid=0, stats=False)


# ------------------------------------------------------------------------------------------------ inputs
def structured(kind, B, Cin, H, W, g):
    """_structured of tests/test_gpu_parity.py on an H x W plane: inputs on which operand-representation errors do not average out."""
    x = torch.randn(B, Cin, H, W, generator=g)
    if kind == "const":
        x = torch.randn(B, Cin, 1, 1, generator=g).expand(B, Cin, H, W).contiguous() * 3.0
    elif kind == "dominant":
        x[:, 3] *= 1.0e4
    elif kind == "cancel":
        x[:, 1::2] = x[:, 0::2]
    else:
        assert kind == "gauss", kind
    return x


def pair_weights(w):
    """_pair_weights of tests/test_gpu_parity.py: pairs cancel to 2^-12 of their terms."""
    w = w.clone()
    w[:, 1::2] = -w[:, 0::2] * (1.0 + 2.0 ** -12)
    return w


@functools.lru_cache(maxsize=None)
def _inputs(key):
    c = key
    Cin = c.C0 + c.C1
    g = torch.Generator().manual_seed(4100 + 7 * c.ks + c.H * 3 + c.W)
    x = structured(c.kind, c.B, Cin, c.H, c.W, g)
    w = torch.randn(c.Cout, Cin, c.ks, c.ks, generator=g) / (Cin * c.ks * c.ks) ** 0.5
    if c.kind == "cancel":
        w = pair_weights(w)
    bias = 0.1 * torch.randn(c.Cout, generator=g)
    coef = None
    if c.coef:
        coef = torch.stack([1 + 0.3 * torch.randn(c.B, Cin, generator=g), 0.3 * torch.randn(c.B, Cin, generator=g)], dim=-1)
        if c.kind == "cancel":                   # paired channels share their (A, B): a prologue must not undo the cancellation
            coef[:, 1::2] = coef[:, 0::2]
        coef = coef.contiguous()
    res = torch.randn(c.B, c.Cout, c.H, c.W, generator=g) if c.res else None
    x0 = x[:, :c.C0].contiguous()
    x1 = x[:, c.C0:].contiguous() if c.C1 else None
    return dict(x0=x0, x1=x1, w=w, bias=bias, coef=coef, res=res, scale=RES_SCALE if c.res else 1.0)


def inputs(c):
    """The fp32 tensors of a case (shared between the cases that differ in the kernel only; do not write to them)."""
    return _inputs(data_key(c))


def activated(c):
    """cat(x0, x1), then A x + B, then x sigmoid(x), all in float64."""
    t = inputs(c)
    xin = (torch.cat([t["x0"], t["x1"]], 1) if t["x1"] is not None else t["x0"]).double()
    if c.coef:
        cf = t["coef"].double()
        xin = cf[..., 0][:, :, None, None] * xin + cf[..., 1][:, :, None, None]
    if c.act:
        xin = xin * torch.sigmoid(xin)
    return xin


@functools.lru_cache(maxsize=None)
def _reference(key):
    c = key
    t = inputs(c)
    xin = activated(c)
    w, bias = t["w"].double(), t["bias"].double()
    scale = float(torch.tensor(t["scale"], dtype=torch.float32).double())           # float64(float32(scale)): what the kernel multiplies by
    conv = F.conv2d(xin, w, None, padding=c.ks // 2)
    y = conv + bias.reshape(1, -1, 1, 1)
    m = F.conv2d(xin.abs(), w.abs(), None, padding=c.ks // 2) + bias.abs().reshape(1, -1, 1, 1)
    if c.res:
        y = y + t["res"].double()
        m = m + t["res"].double().abs()
    return y * scale, (m * scale).max().item()


def reference(c):
    """The case in float64: conv2d(padding = ks // 2) of the activated input, + bias, + res, * float64(float32(scale))."""
    return _reference(data_key(c))[0]


def mag(c):
    """max (conv2d(|xin|, |w|) + |bias| + |res|) * scale: the magnitude of the terms that are summed, the scale fp32 rounding errors are
    proportional to (the normaliser of test_conv_bf16x3_is_fp32_accurate, extended by the bias and the residual)."""
    return _reference(data_key(c))[1]


def f16x1_bound(c):
    """Per-element bound on |y - y64| of the one-piece ids, as test_forced_one_piece_kernel_meets_the_derived_bound applies it: the bound
    of tests/f16x1_ref.py on the bias-free product plus 2^-23 |bias| for the two roundings of the bias add.  With a residual the epilogue
    rounds twice more (the add, the multiplication by the scale), each by at most 2^-24 of its result: 2^-23 (|conv + bias| + |res|),
    and the whole is multiplied by the scale."""
    from tests import f16x1_ref as R
    t = inputs(c)
    d = activated(c)
    _, bound = R.wino_f16x1(d, t["w"])
    bias = t["bias"].double().reshape(1, -1, 1, 1)
    bound = bound + 2.0 ** -23 * bias.abs()
    if c.res:
        pre = F.conv2d(d, t["w"].double(), None, padding=1) + bias
        bound = (bound + 2.0 ** -23 * (pre.abs() + t["res"].double().abs())) * t["scale"]
    return bound


# ------------------------------------------------------------------------------------------------ which kernel must run
def kernel_table():
    """{id: (family, ks, pieces, kparts, own_cot, weights, fallback ids)} parsed from kConvKernels."""
    src = open(WR.HEADER).read()
    enum = dict((n, int(v)) for n, v in re.findall(r"\b(CK_\w+) = (-?\d+)", src))
    body = src[src.index("kConvKernels[] = {"):src.index("kNoConvKernel")]
    rows = {}
    for name, fam, ks, pc, kp, own, wt, fb in re.findall(
            r"\{(CK_\w+),\s*\"\w+\",\s*CF_(\w+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(true|false),\s*(CW_\w+),[^{]*\{([^}]*)\}", body):
        rows[enum[name]] = (fam, int(ks), int(pc), int(kp), own == "true", wt, [enum[t.strip()] for t in fb.split(",") if t.strip() != "-1"])
    return rows


DIRECT = (0, 1, 2, 3)
WINO_FAMILIES = ("WINO", "WINO2H", "WINO3", "WINO3P", "WINO1H")


def dispatcher_ids():
    """The ids a launch can end in: everything in the header but the GEMM forms of a 3x3, which the model launches itself."""
    return sorted(k for k, row in kernel_table().items() if row[0] != "GEMM3")


def conv_cout_tile(Cout):
    return 3 if Cout % 96 == 0 else 4 if Cout % 128 == 0 else 2 if Cout % 64 == 0 else 1


def round_up(a, b):
    return -(-a // b) * b


def launch_geometry(c):
    """(CinP, cot, CoutP) as mcvd_op_conv2d sets them; cot is the direct kernel's tile until a kernel with a tile of its own takes conv_cot."""
    cot = conv_cout_tile(c.Cout)
    return round_up(c.C0 + c.C1, 16 if c.ks == 3 else 32), cot, round_up(c.Cout, 32 * cot)


Q1_PT, Q1_CK, Q1_NB, Q1_MAXIMG = 128, 16, 4, 4
G1_PT, G1_MAXIMG = 128, 4


def q1_lds_bytes(np_, cot, Cin, HW, table):
    nimg = 1 if HW >= Q1_PT else Q1_PT // HW
    pix = Q1_NB * Q1_CK * Q1_PT + (nimg * Cin * 2 if table else 0)
    return max((Q1_NB * (cot * np_ * 256) + pix) * 4, (32 * cot) * (Q1_PT + 4) * 4)


def split1_supported(c, cot, np_):
    """conv1x1_h2_supported for a stand-alone launch (weight pieces present, no im2col form)."""
    CinP, _, CoutP = launch_geometry(c)
    Cin, HW = c.C0 + c.C1, c.H * c.W
    if c.ks != 1 or np_ not in (2, 3) or HW % 32 != 0 or not 1 <= cot <= 4 or (CoutP // 32) % cot != 0:
        return False
    if not (HW % Q1_PT == 0 or (HW < Q1_PT and Q1_PT % HW == 0 and Q1_PT // HW <= Q1_MAXIMG)):
        return False
    if Cin % Q1_CK != 0 or CinP % Q1_CK != 0 or (c.C1 > 0 and c.C0 % Q1_CK != 0):
        return False
    if c.B * max(c.C0, c.C1) * HW >= 1 << 31 or (c.act and not c.coef):
        return False
    return q1_lds_bytes(np_, cot, Cin, HW, c.coef) <= 80 * 1024


def dma1_supported(c, ck, pxw):
    """conv1x1_dma_supported."""
    CinP, _, _ = launch_geometry(c)
    Cin, HW, PT = c.C0 + c.C1, c.H * c.W, G1_PT * pxw
    if c.ks != 1 or HW % 32 != 0 or pxw not in (1, 2) or (pxw == 2 and ck != 16):
        return False
    if not (HW % PT == 0 or (HW < PT and PT % HW == 0 and PT // HW <= G1_MAXIMG)):
        return False
    if Cin % ck != 0 or CinP % ck != 0 or (c.C1 > 0 and c.C0 % ck != 0):
        return False
    return not (c.B * max(c.C0, c.C1) * HW >= 1 << 31 or (c.act and not c.coef))


def usable(kid, c, table=None):
    """conv_kernel_usable(kid) for the stand-alone launch of case c (whose forced id decides which weight images exist and how much room
    the K parts have)."""
    table = table or kernel_table()
    fam, ks, pieces, kparts, own_cot, wt, _ = table[kid]
    fam0, _, _, kp0, own0, wt0, _ = table[c.kid]
    CinP, cot, CoutP = launch_geometry(c)
    if own0 and c.cot > 0:
        cot = c.cot
    if fam in WINO_FAMILIES:
        if c.ks != 3 or fam0 not in WINO_FAMILIES:
            return False
        # mcvd_op_conv2d packs the fp32 Winograd image and the forced id's own; id 4 is handed no K split
        return WR.admits(fam, c.C0 + c.C1, CinP, WR.kernel_parts(fam, kparts if kid != 4 else 0), (c.H, c.W), C0=c.C0, B=c.B, Cout=c.Cout,
                         CoutP=CoutP, weights=wt in (wt0, "CW_WPW"), part_floats=kp0 * c.B * c.Cout * c.H * c.W)
    if fam == "SPLIT1":
        return kid == c.kid and split1_supported(c, cot, pieces)
    if fam == "DMA1":
        return dma1_supported(c, 32 if kid == 6 else 16, 2 if kid == 9 else 1) and not (kid == 6 and cot == 9)
    return False


def tile_fits(kid, c):
    """launch_conv_mfma's `fits` for the pixel tile of a direct id."""
    bpx = 256 if kid == 0 else 128 if kid == 1 else 64
    if bpx % c.W != 0:
        return False
    rows = bpx // c.W
    return c.H % rows == 0 if rows <= c.H else rows % c.H == 0


def expected_id(c, table=None):
    """The id a launch with conv_shape = c.kid must report: the first entry of that id's fallback list that admits the launch; after the list
    the direct tile -- the forced one where its pixel tile fits the plane, else "direct" (one of 0..3, the heuristic's choice)."""
    table = table or kernel_table()
    for kid in table[c.kid][6]:
        if usable(kid, c, table):
            return kid
    if c.kid in DIRECT and tile_fits(c.kid, c):
        return c.kid
    return "direct"


def ran_as_expected(ran, want):
    return ran in DIRECT if want == "direct" else ran == want


def min_cin(kid, table=None):
    """The fewest input channels at which the Winograd id `kid` itself takes a launch (the rule's min_chunks times the parts); 64 for
    everything else, as the other GPU files."""
    table = table or kernel_table()
    fam, _, _, kparts, _, _, _ = table[kid]
    if fam not in WINO_FAMILIES:
        return 64
    chunk, _, _, min_chunks, _, _ = WR.RULES["WINO2H" if fam == "WINO1H" else fam]
    parts = max(kparts, 1)
    return max(64, chunk * parts * min_chunks[{1: 0, 2: 1, 4: 2, 8: 3}[parts]])
