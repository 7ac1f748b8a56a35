"""CPU: the nearest-neighbour check (evaluation/nearest_neighbor.py:70-114) against what the REAL reference computed
(tests/golden/nearest_neighbor.pt, tools/gen_nearest_neighbor_golden.py) -- no GPU.

  * tests/nn_ref.py (fp64, direct differences, ties to the lower index) reproduces the reference's indices for every row and its
    plot_data exactly, its fp32 min-distances within 8 x the fixture's ref_rel_dev (the reference's own deviation from fp64);
  * the restated merge over pieces and the restated collect step equal the one-shot search and a plain gather;
  * the package's host side -- metrics.NearestNeighbors and runner.nearest_neighbors -- runs for real with the three device calls
    (knn_search, hflip_u8, nn_collect) replaced by the restatement, and is held to the same fixture."""
import numpy as np
import pytest
import torch

from tests import nn_ref
from tests.golden_io import load_golden

NAMES = [c[0] for c in nn_ref.CASES]
_cache = {}


def fixture(golden_dir):
    if "g" not in _cache:
        _cache["g"] = load_golden(golden_dir, "nearest_neighbor.pt")
    return _cache["g"]


def restated(golden_dir, name):
    """One fixture case with its seeded inputs and the fp64 restatement, computed once and shared (the GPU tests read it too)."""
    if name not in _cache:
        g = fixture(golden_dir)["cases"][name]
        c = nn_ref.make_case(name)
        assert abs(float(c["table"].double().sum()) - g["table_sum"]) <= 1e-12 * abs(g["table_sum"]) + 1e-9, "the seeded inputs are not the generator's"
        n, N, k = c["n"], c["N"], c["k"]
        det = nn_ref.TableDetector(c["table"]).eval()
        samples = c["samples"][:n]
        flipped = torch.from_numpy(nn_ref.hflip_u8(samples.numpy()))
        feat_s, feat_f = (det(x)[0].reshape(n, -1).double().numpy() for x in (samples, flipped))
        feat_d = c["table"][:N].double().numpy()
        d2, index, nb, plot = nn_ref.nearest_neighbors(samples.numpy(), c["data"].numpy(), feat_s, feat_f, feat_d, k)
        _cache[name] = dict(c, golden=g, det=det, feat_s=feat_s, feat_f=feat_f, feat_d=feat_d, d2=d2, index=index, neighbors=nb, plot=plot)
    return _cache[name]


def distances_within(got, g):
    """|d - d_ref| <= 8 ref_rel_dev d_ref against the reference's fp32 min-distances."""
    ref = g["distances"].double().numpy()
    return bool((np.abs(np.asarray(got) - ref) <= 8 * g["ref_rel_dev"] * ref).all())


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(golden_dir, name):
    w = restated(golden_dir, name)
    g = w["golden"]
    assert g["nrow"] == w["k"] + 1 and g["min_gap"] >= 8 * g["ref_rel_dev"]
    assert np.array_equal(w["index"], g["indices"].numpy()), "indices, every row"
    assert np.array_equal(w["plot"], g["plot_data"].numpy()), "plot_data"
    dev = np.abs(np.sqrt(w["d2"]) - g["distances"].double().numpy()) / g["distances"].double().numpy()
    print(f"  {name}: distances at most {dev.max() / g['ref_rel_dev']:.3f} x ref_rel_dev {g['ref_rel_dev']:.3e}; min gap {g['min_gap']:.3e}")
    assert distances_within(np.sqrt(w["d2"]), g)
    if name == "mirror":
        from tests import prdc_ref
        one, two = prdc_ref.dist2(w["feat_s"], w["feat_d"]), prdc_ref.dist2(w["feat_f"], w["feat_d"])
        wins = [two[0, j] < one[0, j] for j in w["index"][0]]
        assert any(wins) and not all(wins), "each view wins for a neighbour of sample 0"


@pytest.mark.parametrize("name", NAMES)
def test_restated_pieces_and_collect(golden_dir, name):
    """The merge over pieces of sizes (1, k - 1, the rest) and (64, 64, ...) equals the one-shot search bit for bit, and the collect step
    over those pieces equals a plain gather from the whole set."""
    w = restated(golden_dir, name)
    k, N = w["k"], w["N"]
    for sizes in ([1, k - 1], [64] * (N // 64)):
        d2, index = nn_ref.search_pieces(w["feat_s"], w["feat_d"], k, sizes, w["feat_f"])
        assert np.array_equal(index, w["index"]) and np.array_equal(d2, w["d2"]), sizes
        d2, index, nb, plot = nn_ref.nearest_neighbors(w["samples"][:w["n"]].numpy(), w["data"].numpy(), w["feat_s"], w["feat_f"], w["feat_d"], k, sizes)
        assert np.array_equal(index, w["index"]) and np.array_equal(nb, w["data"].numpy()[w["index"]]) and np.array_equal(plot, w["plot"]), sizes


def test_restated_rules_by_hand():
    """Ties to the lower index, the +inf / -1 tail, the minimum over views, an index_base, and the 8-bit mirror."""
    q = np.array([[0.0, 0.0]])
    r = np.array([[3.0, 4.0], [0.0, 5.0], [1.0, 0.0], [5.0, 0.0]])
    d2, i = nn_ref.search(q, r, 3)
    assert d2.tolist() == [[1.0, 25.0, 25.0]] and i.tolist() == [[2, 0, 1]]
    d2, i = nn_ref.search(q, r[:2], 3, index_base=10)
    assert d2.tolist() == [[25.0, 25.0, np.inf]] and i.tolist() == [[10, 11, -1]]
    d2, i = nn_ref.search(q, r[2:], 3, index_base=12, state=(d2, i))
    assert d2.tolist() == [[1.0, 25.0, 25.0]] and i.tolist() == [[12, 10, 11]]
    d2, i = nn_ref.search(q, r, 2, query2=np.array([[5.0, 1.0]]))
    assert d2.tolist() == [[1.0, 1.0]] and i.tolist() == [[2, 3]]
    x = np.array([[[[0.0, 1.0, 0.5, 128 / 255, 2.0, -1.0]]]], dtype=np.float32)
    assert (nn_ref.hflip_u8(x) * 255).round().tolist() == [[[[0, 255, 128, 127, 255, 0]]]]          # 0.5 * 255 = 127.5 is truncated
    assert nn_ref.min_rel_gap(np.array([[1.0, 2.0, 4.0], [1.0, 1.25, np.inf]])) == 0.2


# ---- the host layer ------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def host_nn_layer(monkeypatch):
    """The three device calls of metrics replaced by the restatement, on CPU tensors; `calls` records the pieces."""
    from mcvd_pytorch_amd import metrics
    calls = []
    monkeypatch.setattr(metrics, "_feature_device", lambda scorenet, *t: torch.device("cpu"))
    monkeypatch.setattr(metrics, "hflip_u8", lambda x, scorenet=None: torch.from_numpy(nn_ref.hflip_u8(x.numpy())))

    def knn_search(query, ref, k=10, query2=None, index_base=0, state=None, scorenet=None):
        assert query.dtype == torch.float32 and ref.dtype == torch.float32, "feature rows are stored as fp32"
        calls.append(dict(rows=len(ref), index_base=index_base, merged=state is not None))
        st = None if state is None else tuple(t.numpy() for t in state)
        d2, i = nn_ref.search(query.double().numpy(), ref.double().numpy(), k, None if query2 is None else query2.double().numpy(), index_base, st)
        return torch.from_numpy(d2), torch.from_numpy(i)

    def nn_collect(held, held_index, new_index, piece, index_base, scorenet=None):
        return torch.from_numpy(nn_ref.collect(None if held is None else held.numpy(), None if held_index is None else held_index.numpy(),
                                               new_index.numpy(), piece.numpy(), index_base))
    monkeypatch.setattr(metrics, "knn_search", knn_search)
    monkeypatch.setattr(metrics, "nn_collect", nn_collect)
    metrics.calls = calls
    yield metrics
    del metrics.calls


def _check(out, w):
    g = w["golden"]
    n, k = w["n"], w["k"]
    assert torch.equal(out["indices"], g["indices"]) and out["distances"].dtype == torch.float64
    assert distances_within(out["distances"].numpy(), g)
    assert torch.equal(out["plot_data"], g["plot_data"])
    assert torch.equal(out["neighbors"], w["data"][g["indices"]]) and tuple(out["neighbors"].shape) == (n, k) + tuple(w["data"].shape[1:])


@pytest.mark.parametrize("name", NAMES)
def test_host_layer_against_the_real_get_nearest_neighbors(golden_dir, tmp_path, host_nn_layer, name):
    """runner.nearest_neighbors on the fixture's inputs: a .pt path of n + 2 samples cut by [:n_samples], the data set as (x, _) batches
    of 128 as the script's DataLoader gives them, out_path."""
    from mcvd_pytorch_amd import nearest_neighbors
    w = restated(golden_dir, name)
    path, out_path = str(tmp_path / "samples_5.pt"), str(tmp_path / "nn.pt")
    torch.save(w["samples"], path)
    batches = [(w["data"][i:i + 128], torch.zeros(1)) for i in range(0, w["N"], 128)]
    out = nearest_neighbors(path, batches, w["det"], k=w["k"], n_samples=w["n"], out_path=out_path)
    _check(out, w)
    assert [c["rows"] for c in host_nn_layer.calls] == [len(b[0]) for b in batches]
    assert [c["index_base"] for c in host_nn_layer.calls] == list(range(0, w["N"], 128)) and [c["merged"] for c in host_nn_layer.calls][0] is False
    saved = torch.load(out_path, weights_only=True)
    assert sorted(saved) == ["distances", "indices", "plot_data"]
    assert all(torch.equal(saved[key], out[key]) for key in saved)


def test_host_layer_forms(golden_dir, host_nn_layer):
    """Bare `x` batches of unequal sizes, a samples tensor, detector results as a list of pooled maps, a bare [b, d] tensor and 4-D maps
    that need the spatial average; update(images, feats=); flip=False; fewer than k rows."""
    from mcvd_pytorch_amd import NearestNeighbors, nearest_neighbors
    w = restated(golden_dir, "cli_default")
    det, n, k, N = w["det"], w["n"], w["k"], w["N"]
    sizes = [1, k - 1, 150, N - 150 - k]
    cuts = np.cumsum([0] + sizes)
    batches = [w["data"][a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    _check(nearest_neighbors(w["samples"], batches, det, k=k, n_samples=n), w)
    seen = []

    def plain(x):                                             # [b, d] itself; the whole batch in one call
        seen.append(len(x))
        return det(x)[0].reshape(len(x), -1)
    _check(nearest_neighbors(w["samples"], batches, plain, k=k, n_samples=n), w)
    assert seen == [n, n] + sizes, "samples, mirrored samples, then every batch whole"
    quarters = torch.tensor([[0.5, -0.5], [-0.5, 0.5]])      # 2 x 2 maps: row + {0.5, -0.5, -0.5, 0.5}, pooled back by the host layer
    maps = lambda x: (det(x)[0] + quarters,)                 # noqa: E731
    out = nearest_neighbors(w["samples"], batches, maps, k=k, n_samples=n)
    assert torch.equal(out["indices"], w["golden"]["indices"])
    # features handed over by the caller: the detector is not called for the data
    nn = NearestNeighbors(w["samples"], det, k=k, n_samples=n)
    nn.detector = None
    for a, b in zip(cuts[:-1], cuts[1:]):
        nn.update(w["data"][a:b], feats=w["table"][a:b])
    _check(nn.result(), w)
    # one view
    one = NearestNeighbors(w["samples"], det, k=k, n_samples=n, flip=False)
    one.update(w["data"])
    want = nn_ref.search(w["feat_s"], w["feat_d"], k)
    assert np.array_equal(one.result()["indices"].numpy(), want[1]) and one.flipped is None
    # below k rows
    few = NearestNeighbors(w["samples"], det, k=k, n_samples=n)
    with pytest.raises(RuntimeError, match=rf"k = {k} neighbours of 0 data rows"):
        few.result()
    few.update(w["data"][:k - 1])
    with pytest.raises(RuntimeError, match=rf"k = {k} neighbours of {k - 1} data rows"):
        few.result()
    few.update(w["data"][k - 1:k])
    assert few.result()["indices"].min() >= 0


def test_host_layer_refusals(golden_dir, host_nn_layer):
    from mcvd_pytorch_amd import NearestNeighbors
    w = restated(golden_dir, "single")
    det, s = w["det"], w["samples"]
    with pytest.raises(ValueError, match="not a .pt or .pth path"):
        NearestNeighbors("samples.npz", det)
    with pytest.raises(ValueError, match=r"image tensor \[n, C, H, W\]"):
        NearestNeighbors(torch.zeros(3, 8), det)
    with pytest.raises(ValueError, match="detector is needed"):
        NearestNeighbors(s, None)
    with pytest.raises(ValueError, match="k = 17 is outside 1..16"):
        NearestNeighbors(s, det, k=17)
    with pytest.raises(ValueError, match="k = 0 is outside 1..16"):
        NearestNeighbors(s, det, k=0)
    with pytest.raises(ValueError, match="no samples"):
        NearestNeighbors(s, det, n_samples=0)
    nn = NearestNeighbors(s, det, k=1, n_samples=1)
    with pytest.raises(ValueError, match="beside samples of shape"):
        nn.update(torch.zeros(4, 1, 8, 8))
    with pytest.raises(ValueError, match="features of shape"):
        nn.update(w["data"][:4], feats=torch.zeros(3, 16))
