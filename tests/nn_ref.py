"""fp64 numpy restatement of get_nearest_neighbors (evaluation/nearest_neighbor.py:70-114) that the device path (mcvd_knn_search,
mcvd_hflip_u8, mcvd_nn_collect; kernels/prdc.cpp) is held to: squared distances by DIRECT differences (prdc_ref.dist2), the minimum over
the two views, a stable sort by (d2, index), the 8-bit mirror, the merge over pieces, the collect step and the plot_data layout -- plus the
seeded inputs and the table detector of the fixture tests/golden/nearest_neighbor.pt.  No GPU, no package import."""
import numpy as np
import torch

from tests import prdc_ref

# (name, N data rows, feature width, n samples, k, channels, seed): the fixture's cases (tools/gen_nearest_neighbor_golden.py)
CASES = [("cli_default", 300, 16, 10, 9, 3, 0), ("wide", 500, 2048, 10, 10, 3, 1), ("k16", 130, 33, 3, 16, 1, 2), ("single", 64, 16, 1, 1, 3, 3),
         ("mirror", 100, 16, 4, 5, 3, 4)]


# ---- the search ------------------------------------------------------------------------------------------------------------------------

def min_dist2(query, ref, query2=None):
    """[Nq, Nr] fp64: the smaller of the squared distances from the query and from its second view."""
    d2 = prdc_ref.dist2(query, ref)
    return d2 if query2 is None else np.minimum(d2, prdc_ref.dist2(query2, ref))


def _select(d2, index, k):
    """The k smallest (d2, index) of every row, ascending, equal d2 lower index first; +inf / -1 where fewer than k exist."""
    Nq = d2.shape[0]
    out_d, out_i = np.full((Nq, k), np.inf), np.full((Nq, k), -1, dtype=np.int64)
    for q in range(Nq):
        live = index[q] >= 0
        d, i = d2[q][live], index[q][live]
        order = np.lexsort((i, d))[:k]                           # primary key d2, then the index
        out_d[q, :len(order)], out_i[q, :len(order)] = d[order], i[order]
    return out_d, out_i


def search(query, ref, k, query2=None, index_base=0, state=None, d2=None):
    """(dist2 [Nq, k] fp64, index [Nq, k] int64) of one call; state = (dist2, index) of earlier calls is merged in."""
    d2 = min_dist2(query, ref, query2) if d2 is None else d2
    index = np.broadcast_to(index_base + np.arange(d2.shape[1], dtype=np.int64), d2.shape)
    if state is not None:
        d2, index = np.concatenate([np.asarray(state[0]), d2], 1), np.concatenate([np.asarray(state[1]), index], 1)
    return _select(d2, index, k)


def search_pieces(query, ref, k, sizes, query2=None, index_base=0):
    """The merge over pieces of the given sizes (the last piece takes the rest)."""
    state, at = None, 0
    for n in list(sizes) + [len(ref)]:
        piece = ref[at:at + n]
        if len(piece):
            state = search(query, piece, k, query2, index_base + at, state)
        at += len(piece)
    return state


def min_rel_gap(d2_sorted):
    """The smallest relative gap between consecutive entries of every row of an ascending [Nq, m] array (finite entries)."""
    a, b = d2_sorted[:, :-1], d2_sorted[:, 1:]
    ok = np.isfinite(b)
    return float(((b - a) / np.where(ok, b, 1.0))[ok].min()) if ok.any() else np.inf


def first_sorted(d2, m):
    return np.sort(d2, axis=1)[:, :m]


def pair_bound(query, ref, index, d, query2=None, index_base=0):
    """[Nq, k]: the derived bound gamma_(d+3) (|a| + |b|)^2 of the Gram form against the direct form for the pair (query i, ref
    index[i, j]); with two views the larger query norm (|min(x, y) - min(x', y')| <= max(|x - x'|, |y - y'|))."""
    nq = np.sqrt((np.asarray(query, dtype=np.float64) ** 2).sum(1))
    if query2 is not None:
        nq = np.maximum(nq, np.sqrt((np.asarray(query2, dtype=np.float64) ** 2).sum(1)))
    nr = np.sqrt((np.asarray(ref, dtype=np.float64) ** 2).sum(1))
    return prdc_ref.gamma(d + 3) * (nq[:, None] + nr[np.maximum(index - index_base, 0)]) ** 2


# ---- the images --------------------------------------------------------------------------------------------------------------------------

def hflip_u8(x):
    """to_tensor(flipper(to_pil(img))): x.mul(255).byte() (fp32 product, truncated; clamped to 0..255), mirrored along W, / 255 in fp32."""
    x = np.asarray(x, dtype=np.float32)
    q = np.clip(x * np.float32(255.0), np.float32(0.0), np.float32(255.0)).astype(np.uint8)
    return q[..., ::-1].astype(np.float32) / np.float32(255.0)


def collect(held, held_index, new_index, piece, index_base):
    """[Nq, k, C, H, W]: slot (q, j) from the piece when new_index[q, j] lies in it, else from the held slot of query q with that index,
    zeros for -1."""
    Nq, k = new_index.shape
    out = np.zeros((Nq, k) + piece.shape[1:], dtype=np.float32)
    for q in range(Nq):
        for j in range(k):
            row = new_index[q, j]
            if index_base <= row < index_base + len(piece):
                out[q, j] = piece[row - index_base]
            elif row >= 0 and held_index is not None:
                at = np.nonzero(held_index[q] == row)[0]
                if len(at):
                    out[q, j] = held[q, at[0]]
    return out


def plot_data(samples, neighbors):
    """[n (k + 1), C, H, W]: sample i followed by its k neighbours (:105-113)."""
    return np.concatenate([np.asarray(samples, dtype=np.float32)[:, None], neighbors], 1).reshape((-1,) + tuple(samples.shape[1:]))


def nearest_neighbors(samples, data, feat_s, feat_f, feat_data, k, sizes=None):
    """The whole function on host arrays: (dist2, index, neighbors, plot_data); `sizes`: the data set in pieces with the collect step."""
    if sizes is None:
        d2, index = search(feat_s, feat_data, k, feat_f)
        nb = np.asarray(data, dtype=np.float32)[np.maximum(index, 0)]
    else:
        state, nb, at = None, None, 0
        for n in list(sizes) + [len(data)]:
            piece = np.asarray(data[at:at + n], dtype=np.float32)
            if len(piece):
                new = search(feat_s, feat_data[at:at + n], k, feat_f, at, state)
                nb = collect(nb, None if state is None else state[1], new[1], piece, at)
                state = new
            at += len(piece)
        d2, index = state
    return d2, index, nb, plot_data(samples, nb)


# ---- the fixture's inputs ----------------------------------------------------------------------------------------------------------------

def _digits(v):
    return [(v >> (4 * j)) & 15 for j in range(4)]


def make_case(name):
    """The seeded inputs of one fixture case: data [N, C, 8, 8] and samples [n + 2, C, 8, 8] (two rows more than n_samples, which
    `[:n_samples]` must drop), values multiples of 1/16 below 1, and the feature table [N + 2 (n + 2), d] fp32 of the TableDetector --
    Gaussian rows: data row j at j, sample i at N + i, its mirrored copy at N + (n + 2) + i.  Every image carries its table row in
    base 16 in the first four pixels of its first line, a sample also the row of its mirrored copy in the last four, right to left.
    Case "mirror": the mirrored copy of sample 0 sits beside data row 7 and sample 0 itself beside data row 3, so each view wins once."""
    _, N, d, n, k, C, seed = next(c for c in CASES if c[0] == name)
    g = torch.Generator().manual_seed(1000 + seed)
    m = n + 2
    data = torch.randint(0, 16, (N, C, 8, 8), generator=g)
    samples = torch.randint(0, 16, (m, C, 8, 8), generator=g)
    table = torch.randn(N + 2 * m, d, generator=g)
    if name == "mirror":
        table[N + m] = table[7] + 0.05 * torch.randn(d, generator=g)
        table[N] = table[3] + 0.05 * torch.randn(d, generator=g)
    for j in range(N):
        data[j, 0, 0, :4] = torch.tensor(_digits(j))
    for i in range(m):
        samples[i, 0, 0, :4] = torch.tensor(_digits(N + i))
        samples[i, 0, 0, 4:] = torch.tensor(_digits(N + m + i)[::-1])
    return dict(name=name, N=N, d=d, n=n, k=k, C=C, seed=seed, data=data.float() / 16.0, samples=samples.float() / 16.0, table=table)


class TableDetector(torch.nn.Module):
    """The stand-in for the reference's InceptionV3([block]) in the nearest-neighbour fixture: called as `model(batch)[0]`, it returns a
    one-element list of [b, d, 1, 1] maps -- row `id` of a feature table, `id` read from the image's first four pixels (base 16,
    round(16 x): the 8-bit round trip of the mirrored copy moves a pixel by less than 1/255).  A lookup is exact on every device, so the
    features of the generator and of a GPU test are the same bits, for the mirrored copies too, whose pixels are no longer multiples of
    1/16 (a convolution of those would depend on the order of its sums)."""

    def __init__(self, table):
        super().__init__()
        self.register_buffer("table", table.float())

    @torch.no_grad()
    def forward(self, x):
        digits = torch.round(x[:, 0, 0, :4] * 16.0).long()
        return [self.table[(digits * torch.tensor([1, 16, 256, 4096], device=x.device)).sum(1)][:, :, None, None]]
