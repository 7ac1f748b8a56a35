"""GPU: fast_fid's device side -- mcvd_knn_radii and mcvd_manifold_hits (kernels/prdc.cpp) through mcvd_pytorch_amd.metrics, and
runner.fast_fid -- against tests/prdc_ref.py (fp64 numpy, direct differences) and what the REAL evaluation/fid_PR.py computed
(tests/golden/fid_pr.pt; the CPU side is tests/test_fid_pr_cpu.py).

Gates:
  * squared radii against the restatement, per row: gamma_(d+3) (|a| + |b|)^2 with the row's norm and the largest norm of the set,
    gamma_n = n 2^-53 / (1 - n 2^-53) -- the Gram form |a|^2 + |b|^2 - 2 a.b against sum (a - b)^2: a dot-product error <= gamma_d |a||b|,
    norm errors <= gamma_d |.|^2 and three additions, for any accumulation order (prdc_ref.radii_bound); derived, not measured;
  * hits: every row equal to the restatement's verdict, after the precondition on the restatement that no verdict changes when the radii
    are scaled by 1 -+ 1e-9 (the inputs hold at 1e-6: tests/test_fid_pr_cpu.py);
  * precision and recall against the reference: 2^-24 relative (its fp32 mean of 0 / 1 values is rounded once);
  * FID: the gate tests/test_gpu_fvd.py applies to frechet_distance against its fixture, rtol_of(full_rank) of tests/test_fvd_cpu.py =
    RTOL_FULL = 1e-10 for statistics of full rank -- the same code path (feature_stats, frechet_from_stats); every set here has N > d.
    Against get_fid_PR's own return value the error of its fp32 mean difference is added (test_fid_pr_cpu.fid_gate).
Measured ratios are printed by every test; on an MI355X the radii reach at most 0.073 of the bound (the forced-split shape; 0.005 at d = 2048)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import prdc_ref
from tests.test_fid_pr_cpu import (PR_RTOL, RTOL_FULL, case_id, fast_fid_config, fid_gate, fixture, pr_cases, restated, stable, within)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {case_id(c): c for c in pr_cases(GOLDEN, seeds=(0,))}          # the four shapes at k = 3 and (67, 259, 5) at k = 1 and k = 7
FORCED = dict(Nr=4099, Ng=4099, d=8, seed=3, k=3)                        # 65 owner blocks, 8 splits of up to 9 tiles (prdc_ref.split_plan)
DTYPES = [torch.float32, torch.float64]


def _radii_ratio(got, x64, k, d, want=None):
    want = prdc_ref.knn_radii2(x64, k) if want is None else want
    return float((np.abs(got.cpu().numpy() - want) / prdc_ref.radii_bound(x64, d)).max())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("cid", list(CASES))
def test_radii_and_hits_against_the_restatement(cid, dtype):
    from mcvd_pytorch_amd import knn_radii, manifold_hits, precision_recall
    c = CASES[cid]
    w = restated(c)
    assert stable(w, 1e-9), "precondition: the restatement's verdicts do not depend on the last bits of the radii"
    r, g = w["feat_r"].to(dtype).cuda(), w["feat_g"].to(dtype).cuda()
    r2_r, r2_g = knn_radii(r, c["k"]), knn_radii(g, c["k"])
    assert r2_r.dtype == torch.float64 and tuple(r2_r.shape) == (c["Nr"],) and tuple(r2_g.shape) == (c["Ng"],)
    ratio = max(_radii_ratio(r2_r, w["feat_r"].numpy(), c["k"], c["d"], w["r2_r"]), _radii_ratio(r2_g, w["feat_g"].numpy(), c["k"], c["d"], w["r2_g"]))
    print(f"  {cid} {dtype}: radii at most {ratio:.4f} of the bound")
    assert ratio <= 1.0
    p_rows, r_rows = manifold_hits(g, r, r2_r), manifold_hits(r, g, r2_g)
    assert p_rows.dtype == torch.bool and tuple(p_rows.shape) == (c["Ng"],) and tuple(r_rows.shape) == (c["Nr"],)
    assert np.array_equal(p_rows.cpu().numpy(), w["p_rows"]) and np.array_equal(r_rows.cpu().numpy(), w["r_rows"])
    assert bool(p_rows[-1]) and bool(r_rows[5]), "the duplicated row is a hit"
    # the restatement's radii instead of the device's: the same verdicts
    assert torch.equal(manifold_hits(g, r, torch.from_numpy(w["r2_r"])), p_rows)
    # end to end, against the reference
    precision, recall, p2, r2 = precision_recall(r, g, c["k"], return_rows=True)
    assert torch.equal(p2, p_rows) and torch.equal(r2, r_rows)
    assert isinstance(precision, float) and within(precision, c["precision"], PR_RTOL) and within(recall, c["recall"], PR_RTOL)
    assert np.array_equal(p_rows.cpu().numpy(), c["p_rows"].numpy().astype(bool)) and np.array_equal(r_rows.cpu().numpy(), c["r_rows"].numpy().astype(bool))


def test_forced_split_shape():
    """d = 8, N = 4099: the split rule gives 8 splits of the swept axis (9 tiles each, the last 2) and 65 owner blocks; the last tile and
    the last block hold three rows."""
    from mcvd_pytorch_amd import knn_radii, manifold_hits
    assert prdc_ref.split_plan(FORCED["Nr"], FORCED["Ng"]) == (65, 65, 9, 8)
    w = restated(FORCED)
    assert stable(w, 1e-9)
    r, g = w["feat_r"].float().cuda(), w["feat_g"].float().cuda()
    r2_r, r2_g = knn_radii(r, 3), knn_radii(g, 3)
    ratio = max(_radii_ratio(r2_r, w["feat_r"].numpy(), 3, 8, w["r2_r"]), _radii_ratio(r2_g, w["feat_g"].numpy(), 3, 8, w["r2_g"]))
    print(f"  forced split: radii at most {ratio:.4f} of the bound")
    assert ratio <= 1.0
    assert np.array_equal(manifold_hits(g, r, r2_r).cpu().numpy(), w["p_rows"]) and np.array_equal(manifold_hits(r, g, r2_g).cpu().numpy(), w["r_rows"])


def test_edge_shapes():
    """N = k + 1 (the radius is the largest distance of the row), Nq = 1, a query set in two calls, mixed dtypes, and rows that are a
    column slice of a wider matrix (ld > d, read in place)."""
    from mcvd_pytorch_amd import knn_radii, manifold_hits
    c = CASES["67x259x5_s0_k3"]
    w = restated(c)
    r64, g64 = w["feat_r"], w["feat_g"]
    for k in (1, 3, 7):
        x = r64[:k + 1]
        got = knn_radii(x.cuda(), k)
        want = prdc_ref.dist2(x.numpy(), x.numpy()).max(axis=1)
        assert _radii_ratio(got, x.numpy(), k, 5, want) <= 1.0, k
    r, g = r64.cuda(), g64.cuda()
    rad = knn_radii(r, 3)
    full = manifold_hits(g, r, rad)
    assert torch.equal(manifold_hits(g[:1], r, rad), full[:1]) and torch.equal(manifold_hits(g[-1:], r, rad), full[-1:])
    assert torch.equal(torch.cat([manifold_hits(g[:100], r, rad), manifold_hits(g[100:], r, rad)]), full), "feat_g in two calls"
    assert torch.equal(manifold_hits(g.float(), r, rad), full) and torch.equal(manifold_hits(g, r.float(), rad), full), "mixed dtypes"
    for dtype in DTYPES:
        wide_r = torch.cat([torch.full((len(r), 2), 9.0), r64, torch.full((len(r), 4), -7.0)], 1).to(dtype).cuda()
        wide_g = torch.cat([g64, torch.full((len(g), 3), 5.0)], 1).to(dtype).cuda()
        rs, gs = wide_r[:, 2:7], wide_g[:, :5]
        assert not rs.is_contiguous() and rs.stride(0) == 11
        assert torch.equal(knn_radii(rs, 3), rad)
        assert torch.equal(manifold_hits(gs, rs, rad), full)


def test_two_calls_are_bit_identical():
    from mcvd_pytorch_amd import knn_radii, manifold_hits
    w = restated(CASES["1031x777x256_s0_k3"])
    r, g = w["feat_r"].float().cuda(), w["feat_g"].float().cuda()
    a, b = knn_radii(r, 3), knn_radii(r, 3)
    assert torch.equal(a, b)
    assert torch.equal(manifold_hits(g, r, a), manifold_hits(g, r, b))


def test_fid_and_fid_pr_against_the_reference(golden_dir, tmp_path):
    """fid_from_features against the real calculate_frechet_distance; fid_pr on images (the stand-in detector's fp32 path is exact, so the
    features are the reference's bit for bit), on a path of features, and fid_from_stats against the real get_fid."""
    from mcvd_pytorch_amd import fid_from_features, fid_from_stats, fid_pr
    from mcvd_pytorch_amd.metrics import get_activations
    g = fixture(golden_dir)
    for c in g["fid"]:
        feat_r, feat_g = prdc_ref.make_features(c["seed"], c["Nr"], c["Ng"], c["d"])
        got = fid_from_features(feat_r.cuda(), feat_g.cuda())
        print(f"  fid ({c['Nr']}, {c['Ng']}, {c['d']}): {got!r} against {c['value']!r}: {abs(got - c['value']) / c['value'] / RTOL_FULL:.3f} of the gate")
        assert within(got, c["value"], RTOL_FULL)
    for c in g["fid_pr"]:
        det = prdc_ref.StandInDetector(c["seed"], dims=24, pooled=c["pooled"]).eval()
        real, fake = prdc_ref.make_images(c["seed"], c["n_real"]), prdc_ref.make_images(c["seed"] + 100, c["n_fake"], scale=13)
        if c["real_as"] == "path":
            real = str(tmp_path / "real.pt")
            torch.save(c["feat_r"], real)
        saved = str(tmp_path / f"feats_{c['name']}.pt")
        fid, precision, recall = fid_pr(real, fake, det, k=c["k"], batch_size=c["batch_size"], save_feats_path=saved)
        assert torch.equal(torch.load(saved, weights_only=True), c["feat_g"])
        print(f"  fid_pr {c['name']}: fid {fid!r} ({abs(fid - c['fid_stats64']) / c['fid_stats64'] / RTOL_FULL:.3f} of the gate), "
              f"precision {precision!r} recall {recall!r}")
        assert within(precision, c["precision"], PR_RTOL) and within(recall, c["recall"], PR_RTOL)
        assert fid_gate(fid, c)
    c = g["get_fid"]
    det = prdc_ref.StandInDetector(c["seed"], dims=24).eval()
    feats = get_activations(prdc_ref.make_images(c["seed"] + 100, c["n_fake"], scale=13), det, 50)
    got = fid_from_stats((c["mu"], c["sigma"]), feats)
    print(f"  get_fid: {got!r} against {c['value']!r}")
    assert within(got, c["value"], RTOL_FULL)


def test_every_refusal():
    """Each MCVD_EINVAL case of the two entries: code -1 with a message, and nothing launched -- the output buffers keep their sentinel."""
    from mcvd_pytorch_amd import _lib, metrics
    dev = torch.device("cuda", torch.cuda.current_device())
    ctx = metrics._package_ctx(dev)
    x = torch.rand(8, 6, device=dev)
    rad = torch.full((8,), -1.0, dtype=torch.float64, device=dev)
    hit = torch.full((8,), 7, dtype=torch.uint8, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731

    def radii(feats=x, dtype=_lib.F32, N=8, d=6, ld=6, k=3, out=rad, ctx=ctx):
        return _lib.lib.mcvd_knn_radii(ctx, P(feats), dtype, N, d, ld, k, P(out))

    def hits(q=x, qd=_lib.F32, Nq=8, ldq=6, r=x, rd=_lib.F32, Nr=8, ldr=6, d=6, radii2=rad, out=hit, ctx=ctx):
        return _lib.lib.mcvd_manifold_hits(ctx, P(q), qd, Nq, ldq, P(r), rd, Nr, ldr, d, P(radii2), P(out))
    bad = [("k = 0", lambda: radii(k=0)), ("k = 8", lambda: radii(k=8)), ("N < k + 1", lambda: radii(N=3)), ("N = 0", lambda: radii(N=0)),
           ("d = 0", lambda: radii(d=0, ld=6)), ("d = 2049", lambda: radii(d=2049, ld=2049)), ("ld < d", lambda: radii(ld=5)),
           ("dtype", lambda: radii(dtype=2)), ("NULL feats", lambda: radii(feats=None)), ("NULL out", lambda: radii(out=None)),
           ("NULL ctx", lambda: radii(ctx=None)),
           ("Nq = 0", lambda: hits(Nq=0)), ("Nr = 0", lambda: hits(Nr=0)), ("hits d = 0", lambda: hits(d=0)), ("hits d = 2049", lambda: hits(d=2049, ldq=2049, ldr=2049)),
           ("ldq < d", lambda: hits(ldq=5)), ("ldr < d", lambda: hits(ldr=5)), ("q dtype", lambda: hits(qd=-1)), ("r dtype", lambda: hits(rd=3)),
           ("NULL query", lambda: hits(q=None)), ("NULL ref", lambda: hits(r=None)), ("NULL radii", lambda: hits(radii2=None)),
           ("NULL hit", lambda: hits(out=None)), ("hits NULL ctx", lambda: hits(ctx=None))]
    for name, call in bad:
        assert call() == -1, name
        assert _lib.last_error(), name
    torch.cuda.synchronize()
    assert bool((rad == -1.0).all()) and bool((hit == 7).all()), "a refused call wrote its output"
    assert radii() == 0 and hits() == 0
    torch.cuda.synchronize()
    assert bool((rad >= 0).all()) and bool((hit <= 1).all())
    with pytest.raises(RuntimeError, match=r"code -1"):
        metrics.knn_radii(x, k=8)
    with pytest.raises(ValueError, match="features"):
        metrics.manifold_hits(x[:, :5], x, rad)


def test_tiny_fast_fid_run(tmp_path):
    """Two checkpoints of the `tiny` net, num_samples = batch_size = 4, a 2-step subsample and a seeded stand-in detector: the result keys,
    finite values, the files, and a second run that reuses the cached features bit for bit without sampling."""
    from mcvd_pytorch_amd import fast_fid, get_model, synthetic
    from tests.test_fid_pr_cpu import cond_batches
    config = fast_fid_config("tiny", num_samples=4, batch_size=4)
    config.device = "cuda:0"
    config.sampling.subsample = 2
    net = get_model(config)
    ckpt_dir, out_dir = tmp_path / "ckpt", tmp_path / "out"
    ckpt_dir.mkdir(), out_dir.mkdir()
    for ckpt, seed in ((100, 1), (200, 2)):
        model = {"module." + k: v for k, v in synthetic.random_state_dict(net, seed=seed).items()}
        torch.save([model, {}, 1, 0, {}], str(ckpt_dir / f"checkpoint_{ckpt}.pt"))
    det = prdc_ref.StandInDetector(5, dims=4, channels=1).cuda().eval()
    seen = []

    def detector(x):
        assert x.is_cuda and x.shape[1:] == (1, 32, 32)
        seen.append(len(x))
        return det(x)
    real = torch.rand(16, 1, 32, 32, generator=torch.Generator().manual_seed(9)).cuda()
    batches = cond_batches(config, 1, 4)
    torch.manual_seed(3)
    out = fast_fid(config, net, real, detector=detector, cond_batches=batches, ckpt_dir=str(ckpt_dir), out_dir=str(out_dir), log=print)
    assert list(out) == ["fids", "precisions", "recalls"] and all(list(v) == [100, 200] for v in out.values())
    assert seen == [16, 8, 16, 8]                                            # 4 rows of 2 frames = 8 images per checkpoint
    for v in out.values():
        assert all(isinstance(x, float) and np.isfinite(x) for x in v.values())
    assert all(0.0 <= out[k][c] <= 1.0 for k in ("precisions", "recalls") for c in (100, 200))
    for ckpt in (100, 200):
        s = torch.load(str(out_dir / f"samples_{ckpt}.pt"), weights_only=True)
        f = torch.load(str(out_dir / f"feats_{ckpt}.pt"), weights_only=True)
        assert tuple(s.shape) == (8, 1, 32, 32) and not s.is_cuda and float(s.min()) >= 0.0 and float(s.max()) <= 1.0 and tuple(f.shape) == (8, 4)
    assert not torch.equal(torch.load(str(out_dir / "samples_100.pt"), weights_only=True), torch.load(str(out_dir / "samples_200.pt"), weights_only=True))
    seen.clear()

    def never(*a, **k):
        raise AssertionError("the second run sampled")
    again = fast_fid(config, net, real, detector=detector, cond_batches=batches, ckpt_dir=str(ckpt_dir), out_dir=str(out_dir), sampler=never, log=print)
    assert seen == [16, 16], "only the real images go through the detector again"
    assert again == out, "the cached features give other numbers"
