"""Golden results of the nearest-neighbour check as the REAL reference computes it -- build container only (needs the reference checkout,
Pillow, scipy and scikit-learn).

    PYTHONDONTWRITEBYTECODE=1 python -m tools.gen_nearest_neighbor_golden

Modelled on tools/gen_fid_pr_golden.py.  The real evaluation/nearest_neighbor.py is imported and its get_nearest_neighbors runs on the CPU
(cuda=False): the sweep over the data set, torch.load(path)[:n_samples], the mirrored copies, get_activations, torch.cdist twice,
torch.min, topk and the plot_data layout are the reference's own code.  Replaced from the outside:
  * the absent `torchvision` -> the inert stand-in modules of oracle/gen_runner_golden.py; `datasets.ffhq` (imported for the script's
    __main__ alone) -> an inert module;
  * `InceptionV3` (pretrained weights that are fetched from the network) -> tests/nn_ref.py's TableDetector, an exact lookup of seeded
    Gaussian feature rows; what is compared is the path around the detector;
  * `save_image` -> a function that keeps plot_data and nrow; `torch.topk` -> the real one, recording its argument and its result;
  * the three torchvision transforms that the function really executes, ToPILImage, RandomHorizontalFlip(p=1.) and ToTensor, are RESTATED
    here with Pillow, they are not the real ones: Image.fromarray of img.mul(255).byte() (HWC; one channel as mode L),
    transpose(FLIP_LEFT_RIGHT), and the uint8 array back to CHW float / 255 -- what torchvision's functional to_pil_image, hflip and
    to_tensor do for float tensors and PIL images of these modes.

Rank stability is a condition on the inputs: nothing is written unless, in every case and for every row, the reference's indices are those
of the fp64 restatement (tests/nn_ref.py, direct differences, ties to the lower index) and the smallest relative gap between consecutive
entries among each row's first k + 1 sorted min-distances is at least 8 x ref_rel_dev, the largest relative deviation of the reference's
fp32 min-distances (all n x N of them) from the restatement's.  In case "mirror" the mirrored view wins for one neighbour of sample 0 and
the unmirrored view for another.

tests/golden/nearest_neighbor.pt (data only; the inputs are rebuilt from their seeds by nn_ref.make_case):
    cases {name: {N, d, n, k, C, seed, plot_data [n (k + 1), C, 8, 8] fp32, nrow, indices [n, k] int64, distances [n, k] fp32 (the
           reference's torch.min values at its indices), ref_rel_dev, min_gap, table_sum (fp64 sum of the feature table: a check that the
           seeded inputs are rebuilt as they were)}}
"""
import os
import sys
import tempfile
import types
from unittest import mock

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from oracle.gen_runner_golden import OUT, REF, _StandIn  # noqa: E402
from tests import nn_ref, prdc_ref  # noqa: E402


def import_real_nearest_neighbor():
    if not any(isinstance(f, _StandIn) for f in sys.meta_path):
        sys.meta_path.insert(0, _StandIn())
    if REF not in sys.path:
        sys.path.insert(0, REF)
    inert = {"datasets": mock.MagicMock(name="datasets"), "datasets.ffhq": mock.MagicMock(name="datasets.ffhq")}
    inert["datasets"].__path__ = []
    with mock.patch.dict(sys.modules, inert):
        import evaluation.nearest_neighbor as NN
    return NN


class ToPILImage:
    def __call__(self, img):
        a = img.mul(255).byte().permute(1, 2, 0).numpy()
        return Image.fromarray(a[:, :, 0], mode="L") if a.shape[2] == 1 else Image.fromarray(a, mode="RGB")


class RandomHorizontalFlip:
    def __init__(self, p=0.5):
        assert p == 1.0

    def __call__(self, pil):
        return pil.transpose(Image.FLIP_LEFT_RIGHT)


class ToTensor:
    def __call__(self, pil):
        a = np.array(pil, dtype=np.uint8)
        a = a[:, :, None] if a.ndim == 2 else a
        return torch.from_numpy(a).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def run_case(NN, name, tmp):
    c = nn_ref.make_case(name)
    N, n, k = c["N"], c["n"], c["k"]
    det = nn_ref.TableDetector(c["table"]).eval()
    inception = types.SimpleNamespace(BLOCK_INDEX_BY_DIM={2048: 0})
    Inception = mock.MagicMock(side_effect=lambda blocks: det)
    Inception.BLOCK_INDEX_BY_DIM = inception.BLOCK_INDEX_BY_DIM
    saved, topk_calls = {}, []
    real_topk = torch.topk

    def topk(x, k):
        out = real_topk(x, k=k)
        topk_calls.append((x.clone(), out[0].clone(), out[1].clone()))
        return out

    def save_image(tensor, path, nrow=8):
        saved.update(plot_data=tensor.clone(), nrow=nrow, path=path)
    path = os.path.join(tmp, f"samples_{name}.pt")
    torch.save(c["samples"], path)
    batches = [(c["data"][i:i + 128], None) for i in range(0, N, 128)]                  # the script's DataLoader(batch_size=128)
    with mock.patch.object(NN, "InceptionV3", Inception), mock.patch.object(NN, "save_image", save_image), \
            mock.patch.object(NN, "ToPILImage", ToPILImage), mock.patch.object(NN, "RandomHorizontalFlip", RandomHorizontalFlip), \
            mock.patch.object(NN, "ToTensor", ToTensor), mock.patch.object(NN, "tqdm", lambda x, **kw: x), \
            mock.patch.object(torch, "topk", topk):
        NN.get_nearest_neighbors(batches, path, os.path.join(tmp, name), n, k=k, cuda=False)      # the REAL function
    assert len(topk_calls) == n and saved["nrow"] == k + 1 and tuple(saved["plot_data"].shape) == (n * (k + 1), c["C"], 8, 8)
    ref_all = -torch.stack([t[0] for t in topk_calls]).double().numpy()                 # [n, N] the reference's fp32 min-distances
    indices = torch.stack([t[2] for t in topk_calls])
    distances = -torch.stack([t[1] for t in topk_calls])
    # the restatement on the same features
    samples = c["samples"][:n]
    feat_s = det(samples)[0].reshape(n, -1).double().numpy()
    feat_f = det(torch.from_numpy(nn_ref.hflip_u8(samples.numpy())))[0].reshape(n, -1).double().numpy()
    feat_d = c["table"][:N].double().numpy()
    d2 = nn_ref.min_dist2(feat_s, feat_d, feat_f)
    d64 = np.sqrt(d2)
    ref_rel_dev = float((np.abs(ref_all - d64) / d64).max())
    gap = nn_ref.min_rel_gap(nn_ref.first_sorted(d64, k + 1))
    want_d2, want_i = nn_ref.search(None, None, k, d2=d2)
    assert np.array_equal(want_i, indices.numpy()), f"{name}: the fp64 restatement ranks differently"
    assert gap >= 8 * ref_rel_dev, f"{name}: gap {gap:.3e} below 8 x {ref_rel_dev:.3e}: another seed"
    _, _, _, plot = nn_ref.nearest_neighbors(samples.numpy(), c["data"].numpy(), feat_s, feat_f, feat_d, k)
    assert np.array_equal(plot, saved["plot_data"].numpy()), f"{name}: plot_data"
    if name == "mirror":
        one, two = prdc_ref.dist2(feat_s, feat_d), prdc_ref.dist2(feat_f, feat_d)
        wins = [two[0, j] < one[0, j] for j in want_i[0]]
        assert any(wins) and not all(wins), "mirror: both views must win for a neighbour of sample 0"
        assert {3, 7} <= set(want_i[0].tolist())
    sys.stdout.write(f"  {name}: N {N} d {c['d']} n {n} k {k}: ref_rel_dev {ref_rel_dev:.3e}, min gap {gap:.3e} (ratio {gap / ref_rel_dev:.0f})\n")
    return dict(N=N, d=c["d"], n=n, k=k, C=c["C"], seed=c["seed"], plot_data=saved["plot_data"], nrow=saved["nrow"], indices=indices,
                distances=distances, ref_rel_dev=ref_rel_dev, min_gap=gap, table_sum=float(c["table"].double().sum()))


def main():
    NN = import_real_nearest_neighbor()
    with tempfile.TemporaryDirectory() as tmp:
        out = dict(cases={c[0]: run_case(NN, c[0], tmp) for c in nn_ref.CASES})
    path = os.path.join(OUT, "nearest_neighbor.pt")
    torch.save(out, path)
    sys.stdout.write(f"wrote {path} ({os.path.getsize(path)} bytes)\n")


if __name__ == "__main__":
    main()
