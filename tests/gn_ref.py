"""GroupNorm as this project computes it, restated in float64 (plain torch on the CPU; nothing here touches the GPU or the library).

Three pieces of native code have to agree for a fused norm to be right: a conv epilogue's per-(sample, channel) partials (sum, M2) in
ConvArgs::stats, the fold of those partials into the (A, B) table (gn_finalize_kernel, ksplit_reduce_gn_kernel), and the same table from a
pass over the tensor (gn_coef_kernel).  The functions below say what each of them must produce; tests/test_gn_ref_cpu.py holds them to
torch.nn.functional.group_norm and to the oracle, tests/test_gpu_gn_partials.py holds the kernels to them.
"""
import numpy as np
import torch

F64 = torch.float64


def fold_partials(st, HW):
    """[B, C, np, 2] partials (sum_i, M2_i about the partial's own mean), each over HW / np pixels -> per-channel (sum, M2), both [B, C],
    by the exact pairwise identities  N = sum n_i,  mean = sum sum_i / N,  M2 = sum (M2_i + n_i (sum_i / n_i - mean)^2)."""
    st = st.detach().to("cpu", F64)
    np_ = st.shape[2]
    assert HW % np_ == 0, (HW, np_)
    n = HW // np_
    s, m2 = st[..., 0], st[..., 1]
    tot = s.sum(-1)
    mean = tot / HW
    return tot, (m2 + n * (s / n - mean[..., None]) ** 2).sum(-1)


def tensor_moments(x):
    """[B, C, ...] -> per-channel (sum, M2) over the trailing dimensions, in float64."""
    x = x.detach().to("cpu", F64).flatten(2)
    return x.sum(-1), ((x - x.mean(-1, keepdim=True)) ** 2).sum(-1)


def group_moments(sources, HW, groups):
    """Mean and biased variance per (sample, group), both [B, groups], over the virtual channel concat of `sources`.  A source is a tensor
    [B, C, ...] with HW trailing elements, given as such or as ("tensor", x), or partials ("partials", st) with st [B, C, np, 2].
    Sources may have different np; a group may straddle a seam."""
    sums, m2s = [], []
    for src in sources:
        kind, src = src if isinstance(src, tuple) else ("tensor", src)
        assert kind in ("tensor", "partials"), kind
        if kind == "tensor":
            assert src[0, 0].numel() == HW, (tuple(src.shape), HW)
        s, m2 = fold_partials(src, HW) if kind == "partials" else tensor_moments(src)
        sums.append(s)
        m2s.append(m2)
    s, m2 = torch.cat(sums, 1), torch.cat(m2s, 1)
    B, C = s.shape
    assert C % groups == 0, (C, groups)
    gs = C // groups
    s, m2 = s.view(B, groups, gs), m2.view(B, groups, gs)
    N = gs * HW
    mean = s.sum(-1) / N
    M2 = (m2 + HW * (s / HW - mean[..., None]) ** 2).sum(-1)
    return mean, M2 / N


def affine_params(mode, B, C, p0=None, p1=None, emb_off=0):
    """(par0, par1), both [B, C] float64, with norm -> par0 * norm + par1, for the three modes of GnArgs:
      0: plain normalisation;
      1: (1 + scale) * norm + shift, scale = p0[b, emb_off + c], shift = p0[b, emb_off + C + c]  (p0: [B, emb_stride] embedding rows);
      2: weight * norm + bias, weight = p0[c], bias = p1[c]."""
    if mode == 1:
        e = p0.detach().to("cpu", F64)
        return 1.0 + e[:, emb_off:emb_off + C], e[:, emb_off + C:emb_off + 2 * C]
    if mode == 2:
        return p0.detach().to("cpu", F64)[None, :].expand(B, C), p1.detach().to("cpu", F64)[None, :].expand(B, C)
    return torch.ones(B, C, dtype=F64), torch.zeros(B, C, dtype=F64)


def coefficients(mean, var, eps, mode, C, p0=None, p1=None, emb_off=0):
    """The [B, C, 2] table (A, B) with y = A x + B the normalised (and modulated) value, float64; mean and var are [B, groups]."""
    B, G = mean.shape
    gs = C // G
    mean = mean.to(F64).repeat_interleave(gs, 1)
    rstd = (1.0 / torch.sqrt(var.to(F64) + eps)).repeat_interleave(gs, 1)
    par0, par1 = affine_params(mode, B, C, p0, p1, emb_off)
    return torch.stack([rstd * par0, par1 - mean * rstd * par0], -1)


def gate_atol(mean, var, eps, mode, C, p0=None, p1=None, emb_off=0, unit=2e-6):
    """unit * max(1, |mean * rstd * par0|) per channel, [B, C, 1]: the absolute part of the coefficient gate, scaled the way the
    large-mean test scales it (B = par1 - mean * rstd * par0 carries the rounding of that product)."""
    B, G = mean.shape
    gs = C // G
    par0, _ = affine_params(mode, B, C, p0, p1, emb_off)
    t = (mean.to(F64) / torch.sqrt(var.to(F64) + eps)).repeat_interleave(gs, 1) * par0
    return unit * t.abs().clamp(min=1.0)[..., None]


# ---- how many partials per (sample, channel) each kernel writes: the launchers' set_last_conv_stats_np calls, restated.
# id -> (family, K parts), the rows of conv_kernels.h (tests/test_gn_ref_cpu.py compares this table with the header)
KERNELS = {
    0: ("TILE", 0), 1: ("TILE", 0), 2: ("TILE", 0), 3: ("TILE", 0),
    4: ("WINO", 0), 8: ("WINO", 2),
    5: ("DMA1", 0), 6: ("DMA1", 0), 9: ("DMA1", 0),
    10: ("WINO3", 0), 11: ("WINO3", 2), 18: ("WINO3", 4), 19: ("WINO3", 8),
    12: ("WINO2H", 0), 13: ("WINO2H", 2), 26: ("WINO2H", 4),
    14: ("SPLIT1", 0), 15: ("SPLIT1", 0),
    16: ("WINO3P", 0), 17: ("WINO3P", 2), 20: ("WINO3P", 4),
    22: ("GEMM3", 0), 23: ("GEMM3", 0),
    24: ("WINO1H", 0), 25: ("WINO1H", 2), 27: ("WINO1H", 4),
}


def expected_np(kid, H, W, B=1):
    """Partials per (sample, channel) the kernel `kid` writes for an H x W plane; 0: it emits none (the consumer reads the tensor).
    B is accepted for symmetry with the launchers' arguments; no rule depends on it."""
    fam, kparts = KERNELS[kid]
    HW = H * W
    if fam == "TILE":
        # conv_mfma.h, conv_mfma_launch: `if (!SPLIT && a.stats && g.nimg == 1) set_last_conv_stats_np(a.H * a.W / (PXT * 32))`.
        # conv_mfma_dispatch_shape: id 0 is PXT 2 (256-pixel tile), id 1 PXT 1 (128), ids 2 and 3 are the SPLIT (split-K) tiles.
        # nimg = RT / min(RT, H) with RT = BPX / W rows per tile: one image per tile from HW >= BPX = 4 * PXT * 32 pixels.
        if kid >= 2:
            return 0
        pxt = 2 if kid == 0 else 1
        return HW // (pxt * 32) if HW >= 4 * pxt * 32 else 0
    if fam in ("WINO", "WINO2H", "WINO3", "WINO3P", "WINO1H"):
        if kparts >= 2:
            # every K-split launcher returns launch_wino_ksplit_reduce (conv_wino.cpp): `set_last_conv_stats_np(1)` where
            # hw4 == 16 || hw4 == 64 (8x8 and 16x16 planes: the fused reduce + finalize or the reduce pass with statistics),
            # else `if (a.stats) set_last_conv_stats_np(0)`.
            return 1 if HW in (64, 256) else 0
        # conv_wino.cpp launch_conv_wino / conv_wino2h.cpp (both piece counts) / conv_wino3.cpp:
        #   `set_last_conv_stats_np(G8 ? 1 : (a.H / 8) * (a.W / 16))`; conv_wino3p.cpp (no 8x8 form): `(a.H / 8) * (a.W / 16)`.
        return 1 if (H == 8 and W == 8) else (H // 8) * (W // 16)
    if fam == "DMA1":
        # conv1x1_dma.cpp launch_conv1x1_dma, both branches: `set_last_conv_stats_np(a.H * a.W / 32)`.
        return HW // 32
    if fam == "SPLIT1":
        # conv1x1_h2.cpp launch_conv1x1_h2: `if (... (HW >= Q1_PT || HW == 64)) set_last_conv_stats_np(HW >= Q1_PT ? HW / Q1_PT : 1)`, Q1_PT = 128.
        return HW // 128 if HW >= 128 else (1 if HW == 64 else 0)
    # GEMM3 (conv_gemm_forms.cpp): launched by the model with ConvArgs::stats unset; the dispatcher does not serve these ids.
    return 0


# ---- gn_coef_kernel's arithmetic in numpy float32, thread for thread (tests/test_gn_ref_cpu.py: does a data kind separate a right
# kernel from a wrong one?).  `x`: one group's data, flat, a multiple of 4 elements.
_f = np.float32


def _block_sum_256(v):
    """block_sum_256: xor-shuffle tree within each wave of 64, then red[0] + red[1] + red[2] + red[3]."""
    v = v.astype(_f).reshape(4, 64).copy()
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, np.arange(64) ^ o]).astype(_f)
    return _f(_f(_f(v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0])


def _streams(n4):
    """The (float4 index, stream, step) visits of every thread: `for (; i + 256 < n4; i += 512)` two streams, then `if (i < n4)` stream a."""
    t = np.arange(256)
    steps = np.maximum(0, (n4 - 256 - t + 511) // 512)        # iterations of the two-stream loop thread t makes
    out = []
    for k in range(int(steps.max())):
        i = t + 512 * k
        out.append((np.where(k < steps, i, -1), np.where(k < steps, i + 256, -1)))
    tail_i = t + 512 * steps                                   # the thread's i when it leaves the loop
    return out, steps, np.where(tail_i < n4, tail_i, -1)


def emulate_gn_coef_pilot(x, eps):
    """The kernel before the fix: one pilot p = x[0] for the group, sums of (x - p) and (x - p)^2, var = E[(x-p)^2] - E[x-p]^2.
    Returns (mean, rstd) as float32."""
    x = np.asarray(x, _f)
    v = x.reshape(-1, 4)
    n4 = v.shape[0]
    p = v[0, 0]
    s = np.zeros((2, 256), _f)
    q = np.zeros((2, 256), _f)

    def add(k, idx):
        on = idx >= 0
        d = (v[np.where(on, idx, 0)] - p).astype(_f)
        ds = _f(1) * ((d[:, 0] + d[:, 1]).astype(_f) + (d[:, 2] + d[:, 3]).astype(_f)).astype(_f)
        dq = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(_f) + (d[:, 2] * d[:, 2] + d[:, 3] * d[:, 3]).astype(_f)).astype(_f)
        s[k] = np.where(on, (s[k] + ds).astype(_f), s[k])
        q[k] = np.where(on, (q[k] + dq).astype(_f), q[k])

    visits, _, tail = _streams(n4)
    for ia, ib in visits:
        add(0, ia)
        add(1, ib)
    add(0, tail)
    inv_n = _f(1.0) / _f(x.size)
    ds = _f(_block_sum_256((s[0] + s[1]).astype(_f)) * inv_n)
    dq = _f(_block_sum_256((q[0] + q[1]).astype(_f)) * inv_n)
    mean = _f(p + ds)
    var = max(_f(dq - _f(ds * ds)), _f(0))
    return mean, _f(1.0) / np.sqrt(_f(var + _f(eps)))


def emulate_gn_coef_merge(x, eps):
    """The kernel after the fix: every float4 contributes its own mean and M2, a stream merges them into a running (count, mean, M2) with
    the exact pairwise update (r = 1 / (k + 1) correctly rounded here, the hardware reciprocal there), and the block folds the 512 streams
    with gn_finalize_kernel's identities.  Returns (mean, rstd), float32."""
    x = np.asarray(x, _f)
    v = x.reshape(-1, 4)
    n4 = v.shape[0]
    mu = np.zeros((2, 256), _f)
    m2 = np.zeros((2, 256), _f)
    cnt = np.zeros((2, 256), _f)          # float4 blocks merged so far

    def add(k, idx):
        on = idx >= 0
        w = v[np.where(on, idx, 0)]
        m = (_f(0.25) * ((w[:, 0] + w[:, 1]).astype(_f) + (w[:, 2] + w[:, 3]).astype(_f)).astype(_f)).astype(_f)
        d = (w - m[:, None]).astype(_f)
        qq = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(_f) + (d[:, 2] * d[:, 2] + d[:, 3] * d[:, 3]).astype(_f)).astype(_f)
        r = (_f(1.0) / (cnt[k] + _f(1.0))).astype(_f)
        dl = (m - mu[k]).astype(_f)
        nmu = (mu[k] + (dl * r).astype(_f)).astype(_f)
        nm2 = (m2[k] + (qq + ((_f(4.0) - (_f(4.0) * r).astype(_f)).astype(_f) * (dl * dl).astype(_f)).astype(_f)).astype(_f)).astype(_f)
        mu[k] = np.where(on, nmu, mu[k])
        m2[k] = np.where(on, nm2, m2[k])
        cnt[k] = np.where(on, cnt[k] + _f(1.0), cnt[k])

    visits, _, tail = _streams(n4)
    for ia, ib in visits:
        add(0, ia)
        add(1, ib)
    add(0, tail)
    n = (_f(4.0) * cnt).astype(_f)
    tot = _block_sum_256(((n[0] * mu[0]).astype(_f) + (n[1] * mu[1]).astype(_f)).astype(_f))
    mean = _f(tot / _f(x.size))
    da, db = (mu[0] - mean).astype(_f), (mu[1] - mean).astype(_f)
    dev = ((m2[0] + (n[0] * (da * da).astype(_f)).astype(_f)).astype(_f) + (m2[1] + (n[1] * (db * db).astype(_f)).astype(_f)).astype(_f)).astype(_f)
    var = _f(_block_sum_256(dev) / _f(x.size))
    return mean, _f(1.0) / np.sqrt(_f(var + _f(eps)))
