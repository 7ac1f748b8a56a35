"""The one-piece fp16 Winograd conv (conv_wino2h.cpp with NP = 1, context option "f16x1", shape ids 24 / 25) restated in fp64, rounding where the
kernel rounds, with the error bound the kernel is held to.  A helper of tests/test_f16x1_arithmetic_cpu.py, tests/test_gpu_f16x1.py and
tools/gen_f16x1_golden.py; no GPU.

The kernel computes, per output tile of 2 x 2 pixels and with K = Cin input channels,

    y = A^T [ sum_c  fp16(U_c * s) (.) fp16(16 * V_c) ] A / (16 s)          U_c = G g_c G^T,   V_c = B^T d_c B

  * s is the layer's power-of-two weight scale (pack_wino2h_weight_kernel: 2.25 |w|max s in [2^13, 2^14); |U| <= 2.25 |w|max), 16 the
    activation scale (H2_ACT_SCALE); both are exact, so is the division that takes them out again;
  * d is the ACTIVATED input (after the affine / SiLU prologue), zero padded;
  * fp16(.) is one round-to-nearest-even to 11 significant bits; beyond 65504 it is Inf (nothing clamps: the range guard reports it);
  * every product of two fp16 values is exact in the fp32 accumulator.

The bound.  Write e(v) = |fp16(v) - v|.  For |v| >= 2^-14 (the smallest normal fp16), e(v) <= 2^-11 |v|; below it the fp16 grid has the
fixed spacing 2^-24 and e(v) <= 2^-25.  With u = U s and v = 16 V, one product is off by at most

    e(u) |v| + |u| e(v) + e(u) e(v)  <=  (2^-10 + 2^-22) |u| |v|                                      both operands normal
                                         + 2^-25 (1 + 2^-11) ( [|u| < 2^-14] |v| + |u| [|v| < 2^-14] ) + 2^-50 [both]      the UNDERFLOW term

and the output transform A^T . A (entries 0, +-1) carries a bound on M through as |A|^T . |A|.  That is all there is to the fp64
restatement below.  The kernel on top of it works in fp32: the accumulation of the K products of a position (the classic K 2^-24 of
the summed magnitudes), the weight transform before its rounding, the affine / SiLU of the prologue, the input transform (sums of four
terms whose error is relative to the terms, not to their possibly cancelled sum) and the output transform and epilogue (four more
roundings).  The allowance for all of that is (16 K + 4) 2^-24 of the same magnitude: sixteen times the accumulation bound -- the 16
terms of a 4 x 4 window that one transformed value can draw on -- plus the four roundings behind the contraction.  Together

    |y - y64|  <=  (2^-10 + 2^-22 + (16 K + 4) 2^-24)  |A|^T [ sum_c |U_c| (.) |V_c| ] |A|   +   underflow term

with y64 the fp64 convolution.  For K <= 1024 the first term dominates: this is an 11-bit arithmetic.  The bound is a worst case over the
signs of the roundings; on Gaussian data the errors average out over the 16 K products of an output and the measured worst ratio is a
few per cent of it.
"""
import math

import torch
import torch.nn.functional as F

BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
G = [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]]
AT = [[1, 1, 1, 0], [0, 1, -1, -1]]
ACT_SCALE = 16.0
F16_MIN_NORMAL = 2.0 ** -14


def weight_scale(w):
    """The pack kernel's rule: 2^e with 2.25 * max|w| * 2^e in [2^13, 2^14)  (frexp(2.25 |w|max) = m 2^k, e = 14 - k)."""
    wmax = float(w.detach().abs().max().float())          # the kernel takes the maximum of the fp32 weights
    if not (0.0 < wmax < 3.0e38):
        return 1.0
    _, k = math.frexp(2.25 * wmax)
    return 2.0 ** min(max(14 - k, -60), 60)


def relative_term(K):
    return 2.0 ** -10 + 2.0 ** -22 + (16 * K + 4) * 2.0 ** -24


def activate(x, coef=None, act=0):
    """The conv's prologue in fp64: x * A_c + B_c per (sample, channel), then SiLU."""
    x = x.double()
    if coef is not None:
        c = coef.double()
        x = x * c[..., 0][:, :, None, None] + c[..., 1][:, :, None, None]
    if act:
        x = x * torch.sigmoid(x)
    return x


def wino_f16x1(d, w, want_bound=True):
    """d: activated input [B, K, H, W] (H, W even), w: [Cout, K, 3, 3].  Returns (y, bound): the one-piece result without bias, products
    accumulated in fp64, and the per-element bound on |y - conv64(d, w)| derived above (None unless want_bound)."""
    d, w = d.double(), w.double()
    Bn, K, H, W = d.shape
    Cout = w.shape[0]
    s = weight_scale(w)
    Gm, Bt, At = (torch.tensor(m, dtype=torch.float64) for m in (G, BT, AT))
    Us = torch.einsum("ij,ocjk,lk->iloc", Gm, w, Gm).reshape(16, Cout, K) * s                   # U * scale           [16, Cout, K]
    tiles = F.pad(d * ACT_SCALE, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)                  # [B, K, ty, tx, 4, 4]
    nty, ntx = tiles.shape[2], tiles.shape[3]
    Vs = torch.einsum("ij,bcyxjk,lk->ilcbyx", Bt, tiles, Bt).reshape(16, K, -1)                 # 16 * V              [16, K, tiles]
    Uh, Vh = Us.half().double(), Vs.half().double()                                              # THE roundings (Inf past 65504)

    def back(M):                                                                                 # A^T M A / (16 s) -> NCHW
        M = M.reshape(4, 4, Cout, Bn, nty, ntx)
        return torch.einsum("ij,jkobyx,lk->boyixl", At, M, At).reshape(Bn, Cout, H, W) / (ACT_SCALE * s)

    y = back(torch.matmul(Uh, Vh))
    if not want_bound:
        return y, None
    aU, aV = Us.abs(), Vs.abs()
    subU, subV = ((aU < F16_MIN_NORMAL) & (aU > 0)).double(), ((aV < F16_MIN_NORMAL) & (aV > 0)).double()      # (zero is exact)
    under = 2.0 ** -25 * (1 + 2.0 ** -11) * (torch.matmul(subU, aV) + torch.matmul(aU, subV)) + 2.0 ** -50 * torch.matmul(subU, subV)
    At_abs = At.abs()
    M = relative_term(K) * torch.matmul(aU, aV) + under
    M = M.reshape(4, 4, Cout, Bn, nty, ntx)
    bound = torch.einsum("ij,jkobyx,lk->boyixl", At_abs, M, At_abs).reshape(Bn, Cout, H, W) / (ACT_SCALE * s)
    return y, bound


def conv_f16x1(x, w, b):
    """Drop-in for a 3x3, padding-1 conv2d in the oracle (tools/gen_f16x1_golden.py): the one-piece result in the input's dtype."""
    y, _ = wino_f16x1(x, w, want_bound=False)
    return (y + b.double().reshape(1, -1, 1, 1)).to(x.dtype)
