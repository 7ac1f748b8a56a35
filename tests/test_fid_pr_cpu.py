"""CPU: fast_fid's scoring and loop (evaluation/fid_PR.py, runners/ncsn_runner.py:2432-2586) against what the REAL reference computed
(tests/golden/fid_pr.pt, tools/gen_fid_pr_golden.py) -- no GPU.

  * tests/prdc_ref.py (fp64, direct differences) reproduces the reference's row verdicts exactly and its precision / recall within
    2^-24 relative: the reference returns an fp32 mean of 0 / 1 values, whose sum is exact and whose division is rounded once;
  * the package's host side -- get_activations / fid_pr / precision_recall / fid_from_stats -- runs for real with the three device calls
    (knn_radii, manifold_hits, feature_stats) replaced by the restatement and numpy, and is held to the same fixtures; FID to the
    gate tests/test_fvd_cpu.py holds frechet_distance to on full-rank statistics (RTOL_FULL = 1e-10; every set here has N > d);
  * runner.fast_fid on a plan-only net with a fake sampler and detector."""
import argparse
import os

import numpy as np
import pytest
import torch

from oracle import synth
from tests import prdc_ref
from tests.golden_io import load_golden
from tests.test_fvd_cpu import RTOL_FULL

PR_RTOL = 2.0 ** -24
_cache = {}


def fixture(golden_dir):
    if "g" not in _cache:
        _cache["g"] = load_golden(golden_dir, "fid_pr.pt")
    return _cache["g"]


def pr_cases(golden_dir, seeds=prdc_ref.SEEDS):
    return [c for c in fixture(golden_dir)["pr"] if c["seed"] in seeds]


def case_id(c):
    return f"{c['Nr']}x{c['Ng']}x{c['d']}_s{c['seed']}_k{c['k']}"


def restated(c):
    """The fp64 restatement of one `pr` case, computed once and shared (the GPU tests read it too): feat_r, feat_g (fp64 tensors), the
    squared radii, the pairwise d2 [Ng, Nr] and the row verdicts."""
    key = case_id(c)
    if key not in _cache:
        feat_r, feat_g = prdc_ref.make_features(c["seed"], c["Nr"], c["Ng"], c["d"])
        r, g = feat_r.numpy(), feat_g.numpy()
        r2_r, r2_g = prdc_ref.knn_radii2(r, c["k"]), prdc_ref.knn_radii2(g, c["k"])
        d_gr = prdc_ref.dist2(g, r)
        _cache[key] = dict(feat_r=feat_r, feat_g=feat_g, r2_r=r2_r, r2_g=r2_g, d_gr=d_gr,
                           p_rows=prdc_ref.hits(None, None, r2_r, d2=d_gr), r_rows=prdc_ref.hits(None, None, r2_g, d2=d_gr.T))
    return _cache[key]


def stable(w, eps):
    """The precondition of an exact comparison of verdicts: none changes when every radius is scaled by 1 - eps or 1 + eps."""
    return all(np.array_equal(prdc_ref.hits(None, None, w["r2_r"], s, d2=w["d_gr"]), w["p_rows"])
               and np.array_equal(prdc_ref.hits(None, None, w["r2_g"], s, d2=w["d_gr"].T), w["r_rows"]) for s in (1.0 - eps, 1.0 + eps))


def within(got, want, rtol):
    return abs(got - want) <= rtol * abs(want)


def fid_gate(fid, c):
    """FID of a fid_pr case: RTOL_FULL against the real calculate_frechet_distance on the fp64 statistics of the reference's own features, and
    against get_fid_PR's return value with the error of its own arithmetic added -- it forms mu_r - mu_g and the dot product of the
    difference in fp32 (its features are fp32 arrays, fid_PR.py:295-298; the means themselves are exact for the stand-in's features): one
    rounding of each difference, one of each square and d - 1 additions, at most (d + 3) 2^-24 |mu_r - mu_g|^2."""
    d = c["feat_r"].shape[1]
    return within(fid, c["fid_stats64"], RTOL_FULL) and abs(fid - c["fid"]) <= RTOL_FULL * c["fid"] + (d + 3) * 2.0 ** -24 * c["dmu2"]


def _ids():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    return [case_id(c) for c in pr_cases(here)]


@pytest.mark.parametrize("cid", _ids())
def test_restatement_reproduces_the_reference(golden_dir, cid):
    c = next(c for c in pr_cases(golden_dir) if case_id(c) == cid)
    w = restated(c)
    assert np.array_equal(w["p_rows"], c["p_rows"].numpy().astype(bool)), "precision rows"
    assert np.array_equal(w["r_rows"], c["r_rows"].numpy().astype(bool)), "recall rows"
    p, r = w["p_rows"].sum() / c["Ng"], w["r_rows"].sum() / c["Nr"]
    print(f"  {cid}: precision {p!r} ({c['precision']!r}), recall {r!r} ({c['recall']!r})")
    assert within(p, c["precision"], PR_RTOL) and within(r, c["recall"], PR_RTOL)
    assert stable(w, 1e-6)
    assert w["r_rows"][5] and w["p_rows"][-1], "the duplicated row is a hit on both sides"


def test_restated_radii_are_the_sorted_distances():
    """knn_radii2 on a set small enough to sort by hand, including a duplicated row (radius 0 at k = 1)."""
    x = np.array([[0.0, 0.0], [3.0, 4.0], [0.0, 0.0], [6.0, 8.0]])
    assert prdc_ref.knn_radii2(x, 1).tolist() == [0.0, 25.0, 0.0, 25.0]
    assert prdc_ref.knn_radii2(x, 2).tolist() == [25.0, 25.0, 25.0, 100.0]
    assert prdc_ref.hits(np.array([[3.0, 0.0], [30.0, 0.0]]), x, [0.0, 16.0, 0.0, 1.0]).tolist() == [True, False]      # 16 <= 16: the comparison is <=


def test_split_rule_restated():
    """The shapes the GPU tests rely on: N = 129 is the smallest count with three splits (and more than one owner block); N = 4099 gives
    eight splits of up to nine tiles over 65 owner blocks."""
    assert prdc_ref.split_plan(128, 128) == (2, 2, 1, 2)
    assert prdc_ref.split_plan(129, 129) == (3, 3, 1, 3)
    assert prdc_ref.split_plan(4099, 4099) == (65, 65, 9, 8)
    assert prdc_ref.split_plan(520, 1) == (1, 9, 1, 9)


@pytest.fixture
def host_device_layer(monkeypatch):
    """The three device calls of metrics replaced by the restatement / numpy, on CPU tensors."""
    from mcvd_pytorch_amd import metrics
    monkeypatch.setattr(metrics, "_feature_device", lambda scorenet, *t: torch.device("cpu"))
    monkeypatch.setattr(metrics, "knn_radii", lambda feats, k=3, scorenet=None: torch.from_numpy(prdc_ref.knn_radii2(feats.double().numpy(), k)))
    monkeypatch.setattr(metrics, "manifold_hits", lambda q, r, rad, scorenet=None: torch.from_numpy(
        prdc_ref.hits(q.double().numpy(), r.double().numpy(), rad.numpy())))

    def stats(feats, start=0, step=1, scorenet=None):
        x = torch.as_tensor(feats).double().numpy()[start::step]
        return torch.from_numpy(np.mean(x, axis=0)), torch.from_numpy(np.cov(x, rowvar=False))
    monkeypatch.setattr(metrics, "feature_stats", stats)
    return metrics


def _detector_of(c, seen=None):
    det = prdc_ref.StandInDetector(c["seed"], dims=24, pooled=c["pooled"]).eval()

    def detector(x):
        if seen is not None:
            seen.append(len(x))
        return det(x)
    return detector


def _images_of(c):
    return prdc_ref.make_images(c["seed"], c["n_real"]), prdc_ref.make_images(c["seed"] + 100, c["n_fake"], scale=13)


@pytest.mark.parametrize("name", ["images_pooled", "images_maps", "path_pooled"])
def test_fid_pr_against_the_real_get_fid_PR(golden_dir, tmp_path, host_device_layer, name):
    """Images through the stand-in detector in batches of 50 (128 = 50 + 50 + 28, 64 = 50 + 14), the [0] of its list result, the spatial
    average of its 2 x 2 maps, a .pt path of features, save_feats_path: the reference's features bit for bit (the stand-in's fp32 path is
    exact), its row verdicts, precision and recall, and its FID."""
    metrics = host_device_layer
    c = next(c for c in fixture(golden_dir)["fid_pr"] if c["name"] == name)
    real, fake = _images_of(c)
    seen = []
    det = _detector_of(c, seen)
    if c["real_as"] == "path":
        real = str(tmp_path / "real.pth")
        torch.save(c["feat_r"], real)
    saved = str(tmp_path / "feats.pt")
    fid, precision, recall = metrics.fid_pr(real, fake, det, k=c["k"], batch_size=c["batch_size"], save_feats_path=saved)
    assert seen == ([50, 50, 28] if c["real_as"] == "images" else []) + [50, 14]
    feat_g = torch.load(saved, weights_only=True)
    assert feat_g.dtype == torch.float32 and torch.equal(feat_g, c["feat_g"])
    if c["real_as"] == "images":
        assert torch.equal(metrics.get_activations(real, det, 50), c["feat_r"])
    print(f"  {name}: fid {fid!r} ({c['fid']!r}: {abs(fid - c['fid']) / c['fid']:.2e}), precision {precision!r}, recall {recall!r}")
    assert within(precision, c["precision"], PR_RTOL) and within(recall, c["recall"], PR_RTOL)
    assert fid_gate(fid, c)
    _, _, p_rows, r_rows = metrics.precision_recall(c["feat_r"], c["feat_g"], c["k"], return_rows=True)
    assert torch.equal(p_rows, c["p_rows"].bool()) and torch.equal(r_rows, c["r_rows"].bool())


def test_get_activations_arguments(golden_dir, tmp_path):
    from mcvd_pytorch_amd.metrics import get_activations
    c = fixture(golden_dir)["fid_pr"][0]
    real, _ = _images_of(c)
    seen = []
    feats = get_activations(real[:7], _detector_of(c, seen), batch_size=50)          # batch_size > n shrinks to n (:133-136)
    assert seen == [7] and torch.equal(feats, c["feat_r"][:7])
    seen.clear()
    get_activations(real[:7], _detector_of(c, seen), batch_size=3)
    assert seen == [3, 3, 1]
    plain = lambda x: _detector_of(c)(x)[0].reshape(len(x), -1)                       # noqa: E731  a detector that returns [b, dims] itself
    assert torch.equal(get_activations(real[:7], plain), c["feat_r"][:7])
    f = torch.randn(5, 3)
    assert get_activations(f) is f
    with pytest.raises(ValueError, match="detector"):
        get_activations(real)
    with pytest.raises(ValueError, match="not a .pt"):
        get_activations("features.npz")
    with pytest.raises(ValueError, match="neither features"):
        get_activations(torch.zeros(3))
    with pytest.raises(ValueError, match="batch_size"):
        get_activations(real, _detector_of(c), batch_size=0)
    with pytest.raises(TypeError):
        get_activations(None)


def test_frechet_of_the_feature_sets(golden_dir, host_device_layer):
    """fid_from_features (numpy statistics here, feature_stats on the device) against the real calculate_frechet_distance."""
    for c in fixture(golden_dir)["fid"]:
        feat_r, feat_g = prdc_ref.make_features(c["seed"], c["Nr"], c["Ng"], c["d"])
        got = host_device_layer.fid_from_features(feat_r, feat_g)
        print(f"  ({c['Nr']}, {c['Ng']}, {c['d']}): {got!r} against {c['value']!r}: relative {abs(got - c['value']) / c['value']:.2e}")
        assert within(got, c["value"], RTOL_FULL)


def test_fid_from_stats_against_the_real_get_fid(golden_dir, tmp_path, host_device_layer):
    """The --no_pr branch: (mu, sigma) and an .npz with the reference's keys."""
    metrics = host_device_layer
    c = fixture(golden_dir)["get_fid"]
    det = prdc_ref.StandInDetector(c["seed"], dims=24).eval()
    feats = metrics.get_activations(prdc_ref.make_images(c["seed"] + 100, c["n_fake"], scale=13), det, 50)
    path = str(tmp_path / "stats.npz")
    np.savez(path, mu=c["mu"].numpy(), sigma=c["sigma"].numpy())
    for stats in ((c["mu"], c["sigma"]), path):
        got = metrics.fid_from_stats(stats, feats)
        assert within(got, c["value"], RTOL_FULL), (got, c["value"])
    with pytest.raises(ValueError, match="npz"):
        metrics.fid_from_stats("stats.pt", feats)


# ---- the runner loop -----------------------------------------------------------------------------------------------------------------

def fast_fid_config(name="tiny", num_samples=9, batch_size=4):
    config = synth.make_config(name)
    config.device = torch.device("cpu")
    config.model.ema = False
    config.data.dataset = "StochasticMovingMNIST"
    config.fast_fid = argparse.Namespace(begin_ckpt=100, end_ckpt=200, freq=100, num_samples=num_samples, batch_size=batch_size, pr_nn_k=3,
                                         ensemble=False, verbose=False, n_steps_each=0, step_lr=0.0)
    return config


def write_fast_fid_checkpoints(config, path, seeds={100: 1, 200: 2}):
    for ckpt, seed in seeds.items():
        model = {"module." + k: v for k, v in synth.make_state_dict(config, seed=seed).items()}
        torch.save([model, {}, 1, 0, synth.make_state_dict(config, seed=seed + 10)], os.path.join(path, f"checkpoint_{ckpt}.pt"))


def cond_batches(config, n_batches, rows, seed=0):
    d = config.data
    g = torch.Generator().manual_seed(seed)
    T = d.num_frames_cond + d.num_frames + getattr(d, "num_frames_future", 0)
    return [(torch.rand(rows, T, d.channels, d.image_size, d.image_size, generator=g), torch.zeros(rows)) for _ in range(n_batches)]


class FakeSampler:
    """Records its calls; returns [1, B, C*nf*S*S] like a final_only sampler: z scaled into the network range plus the cond mean."""

    def __init__(self):
        self.calls = []

    def __call__(self, z, scorenet, cond=None, **kw):
        self.calls.append(dict(z=z, cond=cond, kw=kw, first_param=next(iter(scorenet.parameters())).detach().clone()))
        out = 0.3 * z + (0.0 if cond is None else cond.mean(dim=(1, 2, 3), keepdim=True))
        return out.reshape(1, len(z), -1)


def _fake_scores(monkeypatch, calls):
    from mcvd_pytorch_amd import metrics

    def fid_pr(real, fake, detector=None, k=3, batch_size=50, save_feats_path=None, scorenet=None):
        feats = metrics.get_activations(fake, detector, batch_size)
        calls.append(dict(kind="fid_pr", fake=fake, k=k, save_feats_path=save_feats_path, feats=feats))
        if save_feats_path is not None:
            torch.save(feats, save_feats_path)
        return float(feats.double().sum()), 0.5, 0.25

    def fid_from_stats(stats, feats, scorenet=None):
        calls.append(dict(kind="fid_from_stats", stats=stats, feats=feats))
        return float(feats.double().sum())
    monkeypatch.setattr(metrics, "fid_pr", fid_pr)
    monkeypatch.setattr(metrics, "fid_from_stats", fid_from_stats)


def _detector(x):
    return [x.mean(dim=(2, 3), keepdim=True).repeat(1, 3, 1, 1)]


def test_fast_fid_loop(tmp_path, monkeypatch):
    """num_iters = num_samples // batch_size sampler calls per checkpoint, each checkpoint's own weights in the net, the sampler keywords,
    cond through data_transform and conditioning_fn (the loader started over when it runs out, long batches cut), the final
    (-1, C, S, S) reshape, the files, the result keys and the log lines."""
    from mcvd_pytorch_amd import HipScoreNet, fast_fid
    from mcvd_pytorch_amd.runner import conditioning_fn, data_transform
    config = fast_fid_config(num_samples=9, batch_size=4)                  # 9 // 4 = 2 iterations
    ckpt_dir, out_dir = tmp_path / "ckpt", tmp_path / "out"
    ckpt_dir.mkdir(), out_dir.mkdir()
    write_fast_fid_checkpoints(config, str(ckpt_dir))
    net = HipScoreNet(config, plan_only=True)
    batches = cond_batches(config, 3, 5)                                    # 3 batches of 5 rows for 4 calls: one restart, rows cut to 4
    sampler, scores, lines = FakeSampler(), [], []
    _fake_scores(monkeypatch, scores)
    z = {i: torch.randn(4, 2, 32, 32, generator=torch.Generator().manual_seed(50 + i)) for i in range(2)}
    real = torch.randn(10, 3)
    out = fast_fid(config, net, real, detector=_detector, cond_batches=batches, ckpt_dir=str(ckpt_dir), out_dir=str(out_dir),
                   init_noise_fn=lambda i, shape, dev: z[i].reshape(shape), sampler=sampler, log=lines.append)
    assert list(out) == ["fids", "precisions", "recalls"] and all(list(v) == [100, 200] for v in out.values())
    assert len(sampler.calls) == 4
    for n, call in enumerate(sampler.calls):
        ckpt_seed = 1 if n < 2 else 2
        first_name = next(iter(dict(net.named_parameters())))
        assert torch.equal(call["first_param"], synth.make_state_dict(config, seed=ckpt_seed)[first_name]), "states[0] of the checkpoint (no EMA)"
        assert torch.equal(call["z"], z[n % 2])
        assert call["kw"] == dict(cond_mask=None, final_only=True, denoise=True, subsample_steps=10, clip_before=True, verbose=False, gamma=False)
        x = batches[n % 3][0]
        want_cond = conditioning_fn(config, data_transform(config, x), conditional=True)[1][:4]
        assert torch.equal(call["cond"], want_cond) and call["cond"].shape == (4, 2, 32, 32)
    for c, ckpt in enumerate((100, 200)):
        s = scores[c]
        assert s["kind"] == "fid_pr" and s["k"] == 3 and s["save_feats_path"] == str(out_dir / f"feats_{ckpt}.pt")
        assert s["fake"].shape == (16, 1, 32, 32), "8 rows of 2 frames reshaped to (-1, C, S, S)"
        assert float(s["fake"].min()) >= 0.0 and float(s["fake"].max()) <= 1.0, "inverse_data_transform"
        saved = torch.load(str(out_dir / f"samples_{ckpt}.pt"), weights_only=True)
        assert torch.equal(saved, s["fake"])
        assert out["fids"][ckpt] == float(s["feats"].double().sum()) and out["precisions"][ckpt] == 0.5 and out["recalls"][ckpt] == 0.25
        assert lines[c] == "ckpt: {}, fid: {}, precision: {}, recall: {}".format(ckpt, out["fids"][ckpt], 0.5, 0.25)

    # second run: features first (nothing is loaded, sampled or detected), then samples (detected again, features written)
    os.remove(str(out_dir / "feats_200.pt"))
    (ckpt_dir / "checkpoint_100.pt").unlink(), (ckpt_dir / "checkpoint_200.pt").unlink()
    sampler2, scores2 = FakeSampler(), []
    _fake_scores(monkeypatch, scores2)
    out2 = fast_fid(config, net, real, detector=_detector, cond_batches=batches, ckpt_dir=str(ckpt_dir), out_dir=str(out_dir), sampler=sampler2,
                    log=lines.append)
    assert sampler2.calls == []
    assert scores2[0]["fake"] == str(out_dir / "feats_100.pt") and scores2[0]["save_feats_path"] is None
    assert torch.equal(scores2[1]["fake"], scores[1]["fake"]) and scores2[1]["save_feats_path"] == str(out_dir / "feats_200.pt")
    assert out2 == out
    # with every feature file there, neither a detector nor checkpoints nor cond batches are needed
    out3 = fast_fid(config, net, real, out_dir=str(out_dir), log=lines.append)
    assert out3 == out


def test_fast_fid_no_pr_and_ckpts(tmp_path, monkeypatch):
    """no_pr: fid_from_stats on the features of the samples, no precision / recall, no feats file; `ckpts` replaces the config's range;
    without out_dir nothing is written."""
    from mcvd_pytorch_amd import HipScoreNet, fast_fid
    config = fast_fid_config(num_samples=4, batch_size=4)
    config.model.ema = True                                                  # the EMA shadow states[-1], not states[0]
    write_fast_fid_checkpoints(config, str(tmp_path))
    net = HipScoreNet(config, plan_only=True)
    sampler, scores, lines = FakeSampler(), [], []
    _fake_scores(monkeypatch, scores)
    stats = (torch.zeros(3), torch.eye(3))
    before = sorted(os.listdir(tmp_path))
    out = fast_fid(config, net, stats, detector=_detector, cond_batches=cond_batches(config, 1, 4), ckpts=[200], ckpt_dir=str(tmp_path), no_pr=True,
                   sampler=sampler, log=lines.append)
    assert sorted(os.listdir(tmp_path)) == before
    assert list(out["fids"]) == [200] and out["precisions"] == {} and out["recalls"] == {}
    assert len(sampler.calls) == 1 and scores[0]["kind"] == "fid_from_stats" and scores[0]["stats"] is stats
    assert scores[0]["feats"].shape == (8, 3)
    assert lines == ["ckpt: 200, fid: {}".format(out["fids"][200])]
    first_name = next(iter(dict(net.named_parameters())))
    assert torch.equal(sampler.calls[0]["first_param"], synth.make_state_dict(config, seed=12)[first_name])
    assert sampler.calls[0]["z"].shape == (4, 2, 32, 32)                      # the default z: torch.randn of the init shape


def test_fast_fid_deviations_from_the_reference(tmp_path, monkeypatch):
    """The three documented ones: cond_mask=None for an unconditional config (the reference's name is unbound, :2536); the centred gamma
    variate of video_gen for model.gamma (the reference reads an undefined `real`, :2516); ValueError for a short cond batch."""
    from mcvd_pytorch_amd import HipScoreNet, fast_fid
    scores = []
    _fake_scores(monkeypatch, scores)
    real = torch.randn(10, 3)
    # unconditional
    config = fast_fid_config("tiny_uncond", 4, 4)
    write_fast_fid_checkpoints(config, str(tmp_path), {100: 1})
    sampler = FakeSampler()
    fast_fid(config, HipScoreNet(config, plan_only=True), real, detector=_detector, ckpts=[100], ckpt_dir=str(tmp_path), sampler=sampler, log=print)
    assert sampler.calls[0]["cond"] is None and sampler.calls[0]["kw"]["cond_mask"] is None
    # gamma
    config = fast_fid_config("tiny_gamma", 4, 4)
    write_fast_fid_checkpoints(config, str(tmp_path), {100: 1})
    net = HipScoreNet(config, plan_only=True)
    sampler = FakeSampler()
    torch.manual_seed(7)
    fast_fid(config, net, real, detector=_detector, cond_batches=cond_batches(config, 1, 4), ckpts=[100], ckpt_dir=str(tmp_path), sampler=sampler,
             log=print)
    k0, th0 = float(net.k_cum[0]), float(net.theta_t[0])
    torch.manual_seed(7)
    shape = (4, 2, 32, 32)
    want = torch.distributions.gamma.Gamma(torch.full(shape, k0), torch.full(shape, 1.0 / th0)).sample() - k0 * th0
    assert torch.equal(sampler.calls[0]["z"], want) and sampler.calls[0]["kw"]["gamma"] is True
    # a cond batch shorter than fast_fid.batch_size
    config = fast_fid_config("tiny", 4, 4)
    with pytest.raises(ValueError, match="shorter than fast_fid.batch_size"):
        fast_fid(config, HipScoreNet(config, plan_only=True), real, detector=_detector, cond_batches=cond_batches(config, 1, 3), ckpts=[100],
                 ckpt_dir=str(tmp_path), sampler=FakeSampler(), log=print)


def test_fast_fid_refusals(tmp_path):
    """The two NotImplementedErrors and the argument errors, all before a checkpoint is read (there is none) or a sampler runs."""
    from mcvd_pytorch_amd import HipScoreNet, fast_fid
    config = fast_fid_config()
    net = HipScoreNet(config, plan_only=True)
    real, batches = torch.randn(10, 3), cond_batches(config, 1, 4)

    def never(*a, **k):
        raise AssertionError("the sampler ran")
    run = lambda cfg=config, real=real, **kw: fast_fid(cfg, net, real, **dict(dict(detector=_detector, cond_batches=batches,  # noqa: E731
                                                                                   ckpt_dir=str(tmp_path), sampler=never), **kw))
    ens = fast_fid_config()
    ens.fast_fid.ensemble = True
    with pytest.raises(NotImplementedError, match="ensemble"):
        run(ens)
    smld = fast_fid_config()
    smld.model.version = "SMLD"
    with pytest.raises(NotImplementedError, match="SMLD"):
        run(smld)
    small = fast_fid_config(num_samples=3, batch_size=4)
    with pytest.raises(ValueError, match="num_samples"):
        run(small)
    with pytest.raises(ValueError, match="detector"):
        run(detector=None)
    with pytest.raises(ValueError, match="detector"):
        run(real=torch.zeros(4, 3, 8, 8), detector=None, out_dir=str(tmp_path))
    with pytest.raises(ValueError, match="cond_batches"):
        run(cond_batches=None)
    with pytest.raises(ValueError, match="ckpt_dir"):
        run(ckpt_dir=None)
    with pytest.raises(ValueError, match="npz"):
        run(no_pr=True)
    with pytest.raises(ValueError, match=".pt or .pth"):
        run(real="features.npz")
    with pytest.raises(ValueError, match="must be features"):
        run(real=torch.zeros(3))
