"""fp64 numpy restatement of the improved precision / recall of evaluation/fid_PR.py:209-269 (k-nearest-neighbour manifolds) that the
device kernels (kernels/prdc.cpp) are held to, with the DIRECT-DIFFERENCE form of the squared distance, sum (a - b)^2 -- not the Gram
form |a|^2 + |b|^2 - 2 a.b the device uses --, plus the seeded inputs of the tests and the stand-in detector of the fid_pr fixtures.
No GPU, no package import."""
import numpy as np
import torch

U = 2.0 ** -53
SHAPES = [(193, 131, 37), (67, 259, 5), (520, 333, 2048), (1031, 777, 256)]      # (Nr, Ng, d)
SEEDS = (0, 1, 2)


def gamma(n):
    """gamma_n = n u / (1 - n u), u = 2^-53."""
    return n * U / (1.0 - n * U)


def make_features(seed, Nr, Ng, d, dtype=torch.float64):
    """feat_r = |randn(Nr, d)|; feat_g = |randn(Ng, d)| with its first half scaled by 0.8 and shifted by 0.35 sqrt(37 / d); the last row of
    feat_g is a copy of feat_r[5].  Drawn in fp32 (torch.Generator().manual_seed(seed)), so the fp32 and the fp64 inputs hold the same
    numbers."""
    g = torch.Generator().manual_seed(seed)
    feat_r = torch.randn(Nr, d, generator=g).abs()
    feat_g = torch.randn(Ng, d, generator=g).abs()
    half = Ng // 2
    feat_g[:half] = feat_g[:half] * 0.8 + 0.35 * (37.0 / d) ** 0.5
    feat_g[-1] = feat_r[5]
    return feat_r.to(dtype), feat_g.to(dtype)


def dist2(a, b, budget=1 << 21):
    """[Na, Nb] squared distances sum_c (a_ic - b_jc)^2 in fp64, the differences formed first, then squared and summed (torch on the CPU,
    row blocks of about `budget` elements)."""
    a, b = (torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float64))) for v in (a, b))
    out = torch.empty(len(a), len(b), dtype=torch.float64)
    step = max(1, budget // max(1, len(b) * a.shape[1]))
    for i in range(0, len(a), step):
        diff = a[i:i + step, None, :] - b[None, :, :]
        out[i:i + step] = diff.mul_(diff).sum(-1)
    return out.numpy()


def knn_radii2(x, k, d2=None):
    """The (k+1)-th smallest squared distance of every row to all rows, itself included (kthvalue(k + 1) of :251, squared)."""
    d2 = dist2(x, x) if d2 is None else d2
    return np.partition(d2, k, axis=1)[:, k]


def hits(query, ref, ref_radii2, scale=1.0, d2=None):
    """[Nq] bool: some ref row j has dist2(query_i, ref_j) <= scale * ref_radii2[j]  ((dist <= NNk).any(dim=1), :256, :258)."""
    d2 = dist2(query, ref) if d2 is None else d2
    return (d2 <= scale * np.asarray(ref_radii2)[None, :]).any(axis=1)


def precision_recall(feat_r, feat_g, k=3):
    """(precision, recall, precision rows, recall rows) of calculate_precision_recall_full in fp64."""
    r2_r, r2_g = knn_radii2(feat_r, k), knn_radii2(feat_g, k)
    d_gr = dist2(feat_g, feat_r)
    p_rows = hits(None, None, r2_r, d2=d_gr)
    r_rows = hits(None, None, r2_g, d2=d_gr.T)
    return p_rows.sum() / len(p_rows), r_rows.sum() / len(r_rows), p_rows, r_rows


def radii_bound(x, d):
    """Per row, the derived bound on |radii2(Gram form) - radii2(direct form)|: gamma_(d+3) (|a| + |b|)^2 with the largest norms --
    a dot-product error <= gamma_d |a||b|, norm errors <= gamma_d |.|^2 and three additions, for any accumulation order; an order
    statistic moves by no more than the largest movement of the values it is taken from."""
    n = np.sqrt((np.asarray(x, dtype=np.float64) ** 2).sum(1))
    return gamma(d + 3) * (n + n.max()) ** 2


def split_plan(n_swept, n_owner):
    """The split rule of kernels/prdc.cpp (pd_plan), restated: (owner blocks, swept tiles, tiles per split, splits)."""
    colblocks, tiles = -(-n_owner // 64), -(-n_swept // 64)
    want = max(1, min(-(-512 // colblocks), tiles, 256))
    tps = -(-tiles // want)
    return colblocks, tiles, tps, -(-tiles // tps)


class StandInDetector(torch.nn.Module):
    """A small seeded stand-in for the reference's InceptionV3([block]) in the fid_pr fixtures: called as `model(batch)[0]`, it returns a
    one-element list of [b, dims, h, w] maps -- h = w = 1 when `pooled`, else 2 x 2 (the path the reference averages, :157-160).

    Built so that every fp32 operation on its path is EXACT: one convolution with weights and bias in {-1, 0, 1} (drawn from
    torch.Generator().manual_seed(seed): only the seed is stored) on 8 x 8 images whose values are multiples of 1/16 (make_images) -- over
    the whole image when `pooled`, over its four 4 x 4 quarters otherwise, which the caller then averages.  Features are multiples of 2^-6
    below 2^8, so they do not depend on the machine or the order of the sums, and the reference's fp32 np.mean over a power-of-two number
    of rows (get_fid_PR, :296-297) is exact as well: the fixtures' FID is then the value of the fp64 statistics, which is what the device
    computes.  (Random signed sums of all pixels also keep the covariance well conditioned: FID can be held to the full-rank gate.)"""

    def __init__(self, seed, dims=24, channels=3, pooled=True):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.conv = torch.nn.Conv2d(channels, dims, 8) if pooled else torch.nn.Conv2d(channels, dims, 4, stride=4)
        with torch.no_grad():
            self.conv.weight.copy_(torch.randint(-1, 2, self.conv.weight.shape, generator=g).float())
            self.conv.bias.copy_(torch.randint(-1, 2, self.conv.bias.shape, generator=g).float())

    @torch.no_grad()
    def forward(self, x):
        return [self.conv(x)]


def make_images(seed, n, channels=3, size=8, scale=16):
    """[n, channels, size, size] images in [0, 1): multiples of 1/16 below `scale` / 16."""
    return torch.randint(0, scale, (n, channels, size, size), generator=torch.Generator().manual_seed(seed)).float() / 16.0
