"""Golden results of fast_fid's scoring as the REAL reference computes it -- build container only (needs the reference checkout and scipy).

    PYTHONDONTWRITEBYTECODE=1 python -m tools.gen_fid_pr_golden

Modelled on tools/gen_fvd_golden.py.  The real evaluation/fid_PR.py runs: calculate_precision_recall_full and _part (both, and they must
agree), calculate_frechet_distance, get_fid_PR and get_fid.  Replaced from the outside, nothing else:
  * the absent `torchvision` that evaluation/inception.py imports -> the inert stand-in modules of oracle/gen_runner_golden.py;
  * `InceptionV3` (pretrained weights that are fetched from the network) -> tests/prdc_ref.py's StandInDetector(seed), whose fp32 path is
    exact; what is compared is the path around the detector.  Only the seed is stored.
Nothing is written unless, in every case, the reference's fp32 verdicts equal those of the fp64 restatement (tests/prdc_ref.py) row for row
and every verdict of the restatement is unchanged when all radii are scaled by 1 - 1e-6 and by 1 + 1e-6.

tests/golden/fid_pr.pt (recorded results only; the inputs are rebuilt from their seeds):
    pr     [{Nr, Ng, d, seed, k, precision, recall, p_rows, r_rows}] -- prdc_ref.make_features sets; precision / recall are the floats both real
           functions returned, p_rows [Ng] / r_rows [Nr] uint8 the row verdicts of the real calc_cdist_full / kthvalue / <= / any lines
           (:251-258), whose fp32 means are asserted to be those floats;
    fid    [{Nr, Ng, d, seed, value}] -- the real calculate_frechet_distance on np.mean / np.cov of the fp64 features (sets with N > d);
    fid_pr [{name, seed, n_real, n_fake, pooled, real_as, batch_size, k, fid, fid_stats64, dmu2, precision, recall, feat_r, feat_g, p_rows,
           r_rows}] -- the real get_fid_PR on prdc_ref.make_images sets with the stand-in detector (n = 128 / 64: batches of 50, 50, 28 and
           50, 14), `real_as` "images" or "path" (a .pt of feat_r), feat_g as the reference saved it to save_feats_path; fid_stats64 is the
           real calculate_frechet_distance on the fp64 statistics of those features and dmu2 = |mu_r - mu_g|^2 (get_fid_PR itself forms the
           mean difference and its dot product in fp32);
    get_fid {seed, n_fake, mu, sigma, value} -- the real get_fid(stats.npz, fake images) with the .npz's mu / sigma.
"""
import os
import sys
import tempfile
from unittest import mock

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.gen_runner_golden import OUT, REF, _StandIn  # noqa: E402
from tests import prdc_ref  # noqa: E402

K = 3
DIMS = 24
CPU = torch.device("cpu")


def import_real_fid_pr():
    if not any(isinstance(f, _StandIn) for f in sys.meta_path):
        sys.meta_path.insert(0, _StandIn())
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import evaluation.fid_PR as F
    return F


class _Inception:
    """What get_fid_PR / get_fid construct: InceptionV3([BLOCK_INDEX_BY_DIM[dims]]).to(device)."""
    BLOCK_INDEX_BY_DIM = {DIMS: 0}
    seed, pooled = 0, True

    def __new__(cls, blocks):
        return prdc_ref.StandInDetector(cls.seed, dims=DIMS, pooled=cls.pooled).eval()


def _checked_rows(F, feat_r, feat_g, k, precision, recall, what):
    """The row verdicts of the reference's lines :251-258 (fp32), checked against its own means and against the fp64 restatement."""
    NNk_r = F.calc_cdist_full(feat_r, feat_r).kthvalue(k + 1).values
    NNk_g = F.calc_cdist_full(feat_g, feat_g).kthvalue(k + 1).values
    dist_g_r = F.calc_cdist_full(feat_g, feat_r)
    p_rows, r_rows = (dist_g_r <= NNk_r).any(dim=1), (dist_g_r.T <= NNk_g).any(dim=1)
    assert p_rows.float().mean().item() == precision and r_rows.float().mean().item() == recall, what
    r64, g64 = feat_r.double().numpy(), feat_g.double().numpy()
    r2_r, r2_g = prdc_ref.knn_radii2(r64, k), prdc_ref.knn_radii2(g64, k)
    d_gr = prdc_ref.dist2(g64, r64)
    for scale in (1.0, 1.0 - 1e-6, 1.0 + 1e-6):
        assert np.array_equal(prdc_ref.hits(None, None, r2_r, scale, d2=d_gr), p_rows.numpy()), f"{what}: precision rows unstable at {scale}"
        assert np.array_equal(prdc_ref.hits(None, None, r2_g, scale, d2=d_gr.T), r_rows.numpy()), f"{what}: recall rows unstable at {scale}"
    return p_rows.to(torch.uint8), r_rows.to(torch.uint8)


def gen_pr(F):
    out = []
    cases = [(shape, seed, K) for shape in prdc_ref.SHAPES for seed in prdc_ref.SEEDS] + [(prdc_ref.SHAPES[1], 0, 1), (prdc_ref.SHAPES[1], 0, 7)]
    for (Nr, Ng, d), seed, k in cases:
        feat_r, feat_g = prdc_ref.make_features(seed, Nr, Ng, d, torch.float32)
        full = F.calculate_precision_recall(feat_r, feat_g, CPU, k=k)                       # the REAL functions
        part = F.calculate_precision_recall(feat_r, feat_g, CPU, k=k, save_cpu_ram=True)
        assert full == part, (full, part)
        what = f"({Nr}, {Ng}, {d}) seed {seed} k {k}"
        p_rows, r_rows = _checked_rows(F, feat_r, feat_g, k, full[0], full[1], what)
        assert r_rows[5] == 1 and p_rows[-1] == 1, f"{what}: the duplicated row is not a hit"
        out.append(dict(Nr=Nr, Ng=Ng, d=d, seed=seed, k=k, precision=full[0], recall=full[1], p_rows=p_rows, r_rows=r_rows))
        sys.stdout.write(f"  pr {what}: precision {full[0]:.4f} recall {full[1]:.4f}\n")
    return out


def gen_fid(F):
    out = []
    for (Nr, Ng, d) in prdc_ref.SHAPES:
        if min(Nr, Ng) <= d:
            continue
        for seed in prdc_ref.SEEDS[:1]:
            r, g = (t.numpy() for t in prdc_ref.make_features(seed, Nr, Ng, d, torch.float64))
            value = F.calculate_frechet_distance(np.mean(r, axis=0), np.cov(r, rowvar=False), np.mean(g, axis=0), np.cov(g, rowvar=False))
            assert np.isfinite(value) and value > 0
            out.append(dict(Nr=Nr, Ng=Ng, d=d, seed=seed, value=float(value)))
            sys.stdout.write(f"  fid ({Nr}, {Ng}, {d}) seed {seed}: {value!r}\n")
    return out


def gen_fid_pr(F, tmp):
    out = []
    for name, seed, pooled, real_as in (("images_pooled", 21, True, "images"), ("images_maps", 22, False, "images"), ("path_pooled", 23, True, "path")):
        n_real, n_fake = 128, 64
        real, fake = prdc_ref.make_images(seed, n_real), prdc_ref.make_images(seed + 100, n_fake, scale=13)
        _Inception.seed, _Inception.pooled = seed, pooled
        det = prdc_ref.StandInDetector(seed, dims=DIMS, pooled=pooled).eval()
        feat_r = F.calculate_activations(real, det, 50, DIMS, CPU)                          # the REAL function
        arg = real
        if real_as == "path":
            arg = os.path.join(tmp, f"real_{name}.pt")
            torch.save(feat_r, arg)
        saved = os.path.join(tmp, f"feats_{name}.pt")
        with mock.patch.object(F, "InceptionV3", _Inception):
            fid, precision, recall = F.get_fid_PR(arg, fake, CPU, batch_size=50, dims=DIMS, k=K, save_feats_path=saved)      # the REAL function
        feat_g = torch.load(saved)
        for f in (feat_r, feat_g):                           # the stand-in's exactness: multiples of 2^-6 below 2^8, and an exact fp32 column mean
            assert torch.equal(f * 64, (f * 64).round()) and f.abs().max() < 256
            assert np.array_equal(np.mean(f.numpy(), axis=0).astype(np.float64), np.mean(f.double().numpy(), axis=0))
        p_rows, r_rows = _checked_rows(F, feat_r, feat_g, K, precision, recall, name)
        # get_fid_PR forms mu_r - mu_g and its dot product in fp32 (its features are fp32 arrays, :295-298): the same REAL function on the fp64
        # statistics of the same features is recorded beside it, with |mu_r - mu_g|^2, the term that the fp32 arithmetic touches
        r64, g64 = feat_r.double().numpy(), feat_g.double().numpy()
        fid64 = F.calculate_frechet_distance(np.mean(r64, axis=0), np.cov(r64, rowvar=False), np.mean(g64, axis=0), np.cov(g64, rowvar=False))
        dmu2 = float(np.square(np.mean(r64, axis=0) - np.mean(g64, axis=0)).sum())
        assert abs(fid - fid64) <= (DIMS + 3) * 2.0 ** -24 * dmu2, (fid, fid64, dmu2)
        out.append(dict(name=name, seed=seed, n_real=n_real, n_fake=n_fake, pooled=pooled, real_as=real_as, batch_size=50, k=K, fid=float(fid),
                        fid_stats64=float(fid64), dmu2=dmu2,
                        precision=precision, recall=recall, feat_r=feat_r, feat_g=feat_g, p_rows=p_rows, r_rows=r_rows))
        sys.stdout.write(f"  fid_pr {name}: fid {fid!r} precision {precision:.4f} recall {recall:.4f}\n")
    return out


def gen_get_fid(F, tmp):
    seed, n_real, n_fake = 31, 128, 64
    det = prdc_ref.StandInDetector(seed, dims=DIMS).eval()
    feat_r = F.calculate_activations(prdc_ref.make_images(seed, n_real), det, 50, DIMS, CPU).double().numpy()
    mu, sigma = np.mean(feat_r, axis=0), np.cov(feat_r, rowvar=False)
    path = os.path.join(tmp, "stats.npz")
    np.savez(path, mu=mu, sigma=sigma)
    _Inception.seed, _Inception.pooled = seed, True
    with mock.patch.object(F, "InceptionV3", _Inception):
        value = F.get_fid(path, prdc_ref.make_images(seed + 100, n_fake, scale=13), CPU, batch_size=50, dims=DIMS)              # the REAL function
    sys.stdout.write(f"  get_fid: {value!r}\n")
    return dict(seed=seed, n_real=n_real, n_fake=n_fake, mu=torch.from_numpy(mu), sigma=torch.from_numpy(sigma), value=float(value))


def main():
    F = import_real_fid_pr()
    with tempfile.TemporaryDirectory() as tmp:
        out = dict(k=K, dims=DIMS, pr=gen_pr(F), fid=gen_fid(F), fid_pr=gen_fid_pr(F, tmp), get_fid=gen_get_fid(F, tmp))
    path = os.path.join(OUT, "fid_pr.pt")
    torch.save(out, path)
    sys.stdout.write(f"wrote {path} ({os.path.getsize(path)} bytes)\n")


if __name__ == "__main__":
    main()
