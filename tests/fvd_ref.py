"""CPU restatement of the FVD path of video_gen around the detector call (runners/ncsn_runner.py:1918-1982, :2217-2269;
models/fvd/fvd.py:41-49, :160-186, :275-287), and the seeded stand-in detector the fixtures and the tests share.  Besides the kernels
(csrc/kernels/fvd.cpp) this is the one place the arithmetic is written down.

  * axis_table: torch's bilinear source coordinates for one axis of F.interpolate(size=224, mode='bilinear', align_corners=False):
    scale32 = fl32(S) / fl32(224) in fp32; src = fl32(scale32 * (d + 0.5) - 0.5) with ONE rounding (the product and the difference are
    exact in fp64); max(src, 0); i0 = floor(src); i1 = min(i0 + 1, S - 1); l1 = src - i0 in fp32; l0 = 1 - l1 in fp32.
  * preprocess64: preprocess_single for square frames with those fp32 tables and every lerp in fp64:
    ((h0 (w0 p00 + w1 p01) + h1 (w0 p10 + w1 p11)) - 0.5) * 2.  The centre crop of a square frame resized to 224 is the identity.
  * clips64: the clip assembly in front of it -- torch.cat of the parts, [::row_step], to_i3d (grey repeated to RGB, BTCHW -> BCTHW).
  * StandInDetector: NOT the I3D -- a small seeded module with the reference detector's call shape, so that the path around the
    detector can be compared end to end: adaptive average pooling of the clip to (4, 16, 16) per channel (a clip shifted by one pixel
    moves every cell's border, so the features change), a seeded linear layer to 64, tanh, a seeded linear layer to 400.  The
    arithmetic is fp64 and the output is rounded to fp32 once, so CPU and GPU agree up to that one rounding.  Only the seed is stored.
  * make_features: the seeded fp32 Gaussian feature sets of fvd_direct.pt (recipe FEATURE_RECIPE); probe(): what fixtures store in place
    of a whole tensor (its fp64 sum and seeded probe positions with their values).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

OUT = 224
DETECTOR_RECIPE = ("adaptive_avg_pool3d (4, 16, 16) of the fp64 clip -> flatten [3072] -> W1 [64, 3072] = randn * 8 / sqrt(3072), b1 = randn "
                   "-> tanh -> W2 [400, 64] = randn / 8, b2 = randn; fp64 tensors drawn in that order from torch.Generator().manual_seed(seed); "
                   "output rounded to fp32")
FEATURE_RECIPE = ("g = torch.Generator().manual_seed(seed); scale = 0.5 + rand(d); fake = (randn(n_fake, d) * scale * 1.1 + 0.05 * randn(d)).float(); "
                  "real = (randn(n_real, d) * scale).float(); all draws fp64 from g in that order")


@functools.lru_cache(maxsize=None)
def axis_table(S):
    """-> (i0 [224] int64, i1 [224] int64, l0 [224] float32, l1 [224] float32)"""
    scale32 = np.float32(S) / np.float32(OUT)
    d = np.arange(OUT, dtype=np.float64)
    src = (np.float64(scale32) * (d + 0.5) - 0.5).astype(np.float32)          # exact in fp64, then one rounding
    src = np.maximum(src, np.float32(0))
    i0 = np.minimum(np.floor(src).astype(np.int64), S - 1)
    i1 = np.minimum(i0 + 1, S - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    return i0, i1, l0, l1


def axis_table_unfused(S):
    """The WRONG rule (the product rounded to fp32 before the subtraction): what the tests must be able to tell from axis_table."""
    scale32 = np.float32(S) / np.float32(OUT)
    d = np.arange(OUT, dtype=np.float32)
    src = np.maximum(((scale32 * (d + np.float32(0.5))).astype(np.float32) - np.float32(0.5)).astype(np.float32), np.float32(0))
    i0 = np.minimum(np.floor(src).astype(np.int64), S - 1)
    i1 = np.minimum(i0 + 1, S - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, (np.float32(1) - l1).astype(np.float32), l1


def preprocess64(x, table=axis_table):
    """x: [..., S, S] fp32 in [0, 1] -> [..., 224, 224] fp64, preprocess_single's values with the lerps in fp64."""
    S = x.shape[-1]
    assert x.shape[-2] == S, "square frames only"
    i0, i1, l0, l1 = table(S)
    i0, i1 = torch.from_numpy(i0), torch.from_numpy(i1)
    l0, l1 = torch.from_numpy(l0).double(), torch.from_numpy(l1).double()
    x = x.double()
    r0, r1 = x.index_select(-2, i0), x.index_select(-2, i1)
    top = l0 * r0.index_select(-1, i0) + l1 * r0.index_select(-1, i1)
    bot = l0 * r1.index_select(-1, i0) + l1 * r1.index_select(-1, i1)
    v = l0[:, None] * top + l1[:, None] * bot
    return (v - 0.5) * 2


def to_i3d(x, channels):
    """:1918-1923 -- [B, T*C, S, S] -> [B, 3, T, S, S]"""
    x = x.reshape(x.shape[0], -1, channels, x.shape[-2], x.shape[-1])
    if channels == 1:
        x = x.repeat(1, 1, 3, 1, 1)
    return x.permute(0, 2, 1, 3, 4)


def clips64(parts, channels, row_step=1, table=axis_table):
    """parts: [B, T_k*C, S, S] fp32 tensors in clip order -> [ceil(B / row_step), 3, sum T_k, 224, 224] fp64"""
    return preprocess64(to_i3d(torch.cat(list(parts), dim=1)[::row_step], channels), table)


class StandInDetector(torch.nn.Module):
    """A seeded stand-in with the call shape of the reference's detector (models/fvd/fvd.py:43-48): [b, 3, T, H, W] -> [b, 400] fp32."""

    def __init__(self, seed, d=400, hidden=64, grid=(4, 16, 16)):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        n_in = 3 * grid[0] * grid[1] * grid[2]
        self.grid = grid
        self.register_buffer("w1", torch.randn(hidden, n_in, generator=g, dtype=torch.float64) * (8.0 / n_in ** 0.5))
        self.register_buffer("b1", torch.randn(hidden, generator=g, dtype=torch.float64))
        self.register_buffer("w2", torch.randn(d, hidden, generator=g, dtype=torch.float64) / 8.0)
        self.register_buffer("b2", torch.randn(d, generator=g, dtype=torch.float64))

    @torch.no_grad()
    def forward(self, x, rescale=False, resize=False, return_features=True):
        assert not rescale and not resize and return_features and x.dim() == 5 and x.shape[1] == 3
        p = F.adaptive_avg_pool3d(x.double(), self.grid).flatten(1)
        h = torch.tanh(p @ self.w1.t() + self.b1)
        return (h @ self.w2.t() + self.b2).float()


def make_features(seed, d, n_fake, n_real):
    """-> (fake [n_fake, d], real [n_real, d]) fp32, FEATURE_RECIPE"""
    g = torch.Generator().manual_seed(seed)
    scale = 0.5 + torch.rand(d, generator=g, dtype=torch.float64)
    fake = (torch.randn(n_fake, d, generator=g, dtype=torch.float64) * scale * 1.1 + 0.05 * torch.randn(d, generator=g, dtype=torch.float64)).float()
    real = (torch.randn(n_real, d, generator=g, dtype=torch.float64) * scale).float()
    return fake, real


def make_frames(seed, B, TC, S):
    """Seeded frames in [0, 1]: smooth structure plus noise, so that neighbouring pixels differ and a wrong coordinate shows."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(B, TC, S, S, generator=g)
    ramp = torch.linspace(0, 1, S)[None, None, :, None] * torch.linspace(1, 0, S)[None, None, None, :]
    return (0.5 * base + 0.5 * ramp).clamp(0, 1).float()


def probe_index(numel, n, seed):
    return torch.randint(0, numel, (n,), generator=torch.Generator().manual_seed(seed))


def probe(t, n, seed):
    """-> (fp64 sum, probe positions, values there): what a fixture keeps of a tensor too large to store"""
    flat = t.reshape(-1)
    idx = probe_index(flat.numel(), n, seed)
    return float(flat.double().sum()), idx, flat[idx].clone()


def stats_np(feats):
    """compute_stats (fvd.py:275-278)"""
    feats = np.asarray(feats)
    return feats.mean(axis=0), np.cov(feats, rowvar=False)
