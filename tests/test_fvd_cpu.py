"""CPU: the FVD path around the detector -- tests/fvd_ref.py (the restated resize and clip assembly) and mcvd_pytorch_amd.metrics' host
parts (fvd_gates, frechet_from_stats, fvd_stuff / summarize_fvd, VideoMetrics' key groups) against what the REAL preprocess_single,
frechet_distance and NCSNRunner.video_gen computed (fixtures fvd_direct.pt, fvd_runner_{A,B,C}.pt from tools/gen_fvd_golden.py).

Gates:
  * the restatement against the real preprocess_single's probes: the fixture's ref_abs_dev of that case (the restatement's own measured
    distance over the whole tensor when the fixture was made; 1.7e-7 ... 2.3e-7), and the fp64 sum to the same per-element figure;
  * frechet_from_stats on np.mean / np.cov statistics against the real frechet_distance (scipy sqrtm): relative 1e-10 where both
    covariances have full rank, 1e-7 where they are singular (rows <= d: the reference's own sqrtm is then only defined to about
    sqrt(eps)).  Differences measured on these fixtures: 5e-16 ... 3e-15 and 2.5e-9 ... 8.7e-9; a wrong n - 1 or a missing mean term moves
    the value by percent (test_host_frechet_sees_a_wrong_normalisation).  The ratios are printed.
"""
import inspect
import types

import numpy as np
import pytest
import torch

from oracle import synth
from tests import fvd_ref
from tests.golden_io import load_golden

RUNNER_CASES = ("A", "B", "C")
RTOL_FULL, RTOL_SINGULAR = 1e-10, 1e-7
_cache = {}


def direct(golden_dir):
    if "direct" not in _cache:
        _cache["direct"] = load_golden(golden_dir, "fvd_direct.pt")
    return _cache["direct"]


def runner(golden_dir, case):
    if case not in _cache:
        _cache[case] = load_golden(golden_dir, f"fvd_runner_{case}.pt")
    return _cache[case]


def config_of(g):
    """The config of the fixture's run (oracle/gen_runner_golden.py's runner_config fields that the metrics read)."""
    c = synth.make_config(g["config_name"])
    c.data.dataset = "StochasticMovingMNIST"
    c.data.prob_mask_cond, c.data.prob_mask_future, c.data.prob_mask_sync = 0.0, 0.0, False
    for k, v in g["overrides"].items():
        setattr(c.data, k, v)
    c.sampling.fvd, c.sampling.num_frames_pred, c.sampling.preds_per_test = True, g["nfp"], g["preds_per_test"]
    return c


def rtol_of(full_rank):
    return RTOL_FULL if full_rank else RTOL_SINGULAR


def distance_cpu(fake, real, start=0, step=1):
    """frechet_distance with the statistics from numpy (what the device's feature_stats replaces) and the package's host part."""
    from mcvd_pytorch_amd import metrics
    f = np.asarray(torch.as_tensor(fake).double())[start::step]
    r = np.asarray(torch.as_tensor(real).double())
    return metrics.frechet_from_stats(*fvd_ref.stats_np(f), *fvd_ref.stats_np(r))


def features_of(spec):
    fake, real = fvd_ref.make_features(spec["seed"], spec["d"], spec["n_fake"], spec["n_real"])
    for t, (s, idx, values) in ((fake, spec["fake_probe"]), (real, spec["real_probe"])):
        assert torch.equal(t.reshape(-1)[idx], values) and float(t.double().sum()) == s, f"{spec['name']}: the recipe no longer gives the fixture's features"
    return fake, real


def test_restatement_matches_the_real_preprocess_single(golden_dir):
    g = direct(golden_dir)
    assert [(c["S"], c["channels"]) for c in g["resize"]] == [(S, Cc) for S in (11, 48, 64, 128, 256, 300) for Cc in (1, 3)]
    for c in g["resize"]:
        frames = fvd_ref.make_frames(c["frame_seed"], c["B"], c["T"] * c["channels"], c["S"])
        ours = fvd_ref.clips64([frames], c["channels"])
        assert tuple(ours.shape) == (c["B"], 3, c["T"], 224, 224)
        idx = fvd_ref.probe_index(ours.numel(), g["probe_n"], c["probe_seed"])
        dev = (ours.reshape(-1)[idx] - c["values"].double()).abs().max().item()
        dsum = abs(float(ours.sum()) - c["sum"]) / ours.numel()
        print(f"  S {c['S']} C {c['channels']}: probes {dev:.3e} (ref_abs_dev {c['ref_abs_dev']:.3e}), sum per element {dsum:.3e}")
        assert dev <= c["ref_abs_dev"] and dsum <= c["ref_abs_dev"]
        assert c["ref_abs_dev"] <= 1e-6
        if c["channels"] == 1:
            assert torch.equal(ours[:, 0], ours[:, 1]) and torch.equal(ours[:, 0], ours[:, 2])


def test_unfused_coordinate_rule_is_outside_the_gpu_gate_at_128_and_300(golden_dir):
    """8 x ref_abs_dev, the GPU test's gate, lies below what the product-rounded-first rule gives at S = 128 and S = 300."""
    g = direct(golden_dir)
    gate = 8 * g["ref_abs_dev"]
    for c in g["resize"]:
        if c["S"] in (128, 300):
            frames = fvd_ref.make_frames(c["frame_seed"], c["B"], c["T"] * c["channels"], c["S"])
            video = fvd_ref.to_i3d(frames, c["channels"])
            dev = (fvd_ref.preprocess64(video) - fvd_ref.preprocess64(video, fvd_ref.axis_table_unfused)).abs().max().item()
            print(f"  S {c['S']} C {c['channels']}: unfused rule {dev:.3e} against the gate {gate:.3e}")
            assert dev > gate


def test_host_frechet_matches_the_real_frechet_distance(golden_dir):
    g = direct(golden_dir)
    names = [s["name"] for s in g["features"]]
    assert sum(s["full_rank"] for s in g["features"]) == 2 and any(s["step"] == 3 and s["start"] == 1 for s in g["features"]), names
    for spec in g["features"]:
        fake, real = features_of(spec)
        got = distance_cpu(fake, real, spec["start"], spec["step"])
        rel = abs(got - spec["value"]) / spec["value"]
        print(f"  {spec['name']}: {got!r} against {spec['value']!r}: relative {rel:.3e} = {rel / rtol_of(spec['full_rank']):.3f} of the gate")
        assert rel <= rtol_of(spec["full_rank"]), spec["name"]


def test_host_frechet_sees_a_wrong_normalisation(golden_dir):
    """The gates are far below a real error: covariance over n instead of n - 1, or the mean term dropped."""
    from mcvd_pytorch_amd import metrics
    spec = direct(golden_dir)["features"][0]
    fake, real = (t.double().numpy() for t in features_of(spec))
    (mg, sg), (mr, sr) = fvd_ref.stats_np(fake), fvd_ref.stats_np(real)
    biased = metrics.frechet_from_stats(mg, sg * (len(fake) - 1) / len(fake), mr, sr * (len(real) - 1) / len(real))
    no_mean = metrics.frechet_from_stats(mg, sg, mg, sr)
    assert abs(biased - spec["value"]) / spec["value"] > 1e-3 and abs(no_mean - spec["value"]) / spec["value"] > 1e-3


def _cfg(condp, futrf, futrp, sync, condf, nf, nfp, fvd=True):
    ns = types.SimpleNamespace
    return ns(data=ns(channels=1, num_frames_cond=condf, num_frames=nf, num_frames_future=futrf, prob_mask_cond=condp, prob_mask_future=futrp,
                      prob_mask_sync=sync), sampling=ns(fvd=fvd, num_frames_pred=nfp))


# (condp, futrf, futrp, sync, condf, num_frames, num_frames_pred) -> (calc_fvd1, calc_fvd2, calc_fvd3), by hand from ncsn_runner.py:1313-1332
GATE_TABLE = [
    ((0.0, 0, 0.0, False, 2, 2, 8), (True, False, False)),      # :1313-1315 (1) Prediction: condf + nfp = 10
    ((0.0, 0, 0.0, False, 2, 2, 7), (False, False, False)),     # :1314: 9 < 10
    ((0.0, 0, 0.5, False, 2, 2, 8), (True, False, False)),      # :1313: futrf == 0 decides, prob_mask_future is not read
    ((0.0, 1, 0.0, False, 5, 4, 2), (True, False, False)),      # :1316-1318 (1) Interpolation: condf + num_frames + futrf = 10
    ((0.0, 1, 0.0, False, 5, 3, 20), (False, False, False)),    # :1317: 9 < 10, num_frames_pred is not read
    ((0.0, 1, 0.5, False, 1, 8, 9), (True, True, False)),       # :1319-1322 (1) Interp + (2) Pred
    ((0.0, 1, 0.5, False, 1, 8, 8), (True, False, False)),      # :1321: condf + nfp = 9
    ((0.0, 1, 0.5, False, 1, 2, 9), (False, True, False)),      # :1320: 1 + 2 + 1 = 4
    ((0.5, 0, 0.0, False, 2, 2, 8), (True, False, True)),       # :1323-1325 (1) Pred + (3) Gen
    ((0.5, 0, 0.0, False, 2, 2, 7), (False, False, False)),     # :1324
    ((0.5, 1, 0.5, False, 1, 8, 9), (True, True, True)),        # :1326-1328 (1) Interp + (2) Pred + (3) Gen
    ((0.5, 1, 0.5, False, 1, 2, 9), (False, True, True)),       # :1327-1328
    ((0.5, 1, 0.5, True, 1, 8, 9), (True, False, True)),        # :1329-1332 (1) Interp + (3) Gen under prob_mask_sync
    ((0.5, 1, 0.5, True, 1, 8, 5), (True, False, False)),       # :1332: condf + nfp = 6
]


def test_gates_follow_the_runner(golden_dir):
    from mcvd_pytorch_amd import fvd_gates
    for args, want in GATE_TABLE:
        assert fvd_gates(_cfg(*args)) == want, args
        assert fvd_gates(_cfg(*args, fvd=False)) == (False, False, False)
    no_key = _cfg(*GATE_TABLE[0][0])
    del no_key.sampling.fvd
    assert fvd_gates(no_key) == (False, False, False)
    with pytest.raises(ValueError):
        fvd_gates(_cfg(0.5, 1, 0.0, False, 1, 8, 9))            # no branch of :1313-1332: the reference fails on an unbound name
    seen = set()
    for case in RUNNER_CASES:
        g = runner(golden_dir, case)
        assert fvd_gates(config_of(g)) == tuple(g["gates"]), case
        seen.add(tuple(g["gates"]))
    assert seen == {(True, False, False), (True, True, False), (True, False, True)}


def _summary_from_embeddings(g, monkeypatch):
    """VideoMetrics.summary() with the runner's embeddings put in place and the statistics taken from numpy."""
    from mcvd_pytorch_amd import VideoMetrics, metrics
    monkeypatch.setattr(metrics, "frechet_distance", lambda fake, real, start=0, step=1, scorenet=None: distance_cpu(fake, real, start, step))
    vm = VideoMetrics(config_of(g), preds_per_test=g["preds_per_test"], fvd=lambda *a, **kw: None)
    n = len(g["embeddings"]["fake_embeddings"])
    vm.vid[1][0].extend([np.float32(0.01 * (i + 1)) for i in range(n)])
    vm.vid[1][1].extend([0.5 + 0.01 * i for i in range(n)])
    if g["second_calc"]:
        vm.vid[2][0].extend([np.float32(0.02 * (i + 1)) for i in range(n)])
        vm.vid[2][1].extend([0.4 + 0.01 * i for i in range(n)])
    for k, suffix in ((1, ""), (2, "2"), (3, "3")):
        for which, name in ((0, "real"), (1, "fake")):
            e = g["embeddings"][f"{name}_embeddings{suffix}"]
            if len(e):
                vm.emb[k][which].append(e)
    return vm, vm.summary()


@pytest.mark.parametrize("case", RUNNER_CASES)
def test_summary_arithmetic_reproduces_the_runner(golden_dir, case, monkeypatch):
    """fvd / fvd_traj_mean / _std / _conf95 (and the 2 / 3 groups) from the stored embeddings: the runner's values, key names and order."""
    g = runner(golden_dir, case)
    ppt = g["preds_per_test"]
    vm, out = _summary_from_embeddings(g, monkeypatch)
    want_keys = [k for k in g["vid_metrics"] if k != "ckpt" and not k.startswith("lpips")]
    assert list(out) == want_keys, (list(out), want_keys)
    assert [k for k in out if k.startswith("fvd")] == g["fvd_keys"] and g["fvd_keys"]
    d = g["embeddings"]["fake_embeddings"].shape[1]
    for k in g["fvd_keys"]:
        want, got = g["vid_metrics"][k], out[k]
        if ppt == 1 and "traj" in k:
            assert want == -1 and got == -1 and isinstance(got, int)
            continue
        # every embedding set here has fewer rows than d = 400: the singular gate; std and conf95 are differences of such values and are
        # held to the same bound relative to the FVD they are spreads of
        assert len(g["embeddings"]["fake_embeddings"]) <= d
        scale = abs(g["vid_metrics"][k.split("_")[0]]) if ("std" in k or "conf95" in k) else abs(want)
        print(f"  {case} {k}: {got!r} against {want!r}: {abs(got - want) / scale:.3e} (gate {RTOL_SINGULAR})")
        assert abs(got - want) <= RTOL_SINGULAR * scale, k
    e = vm.embeddings()
    assert list(e) == ["real_embeddings", "fake_embeddings", "real_embeddings2", "fake_embeddings2", "real_embeddings3", "fake_embeddings3"]
    for k, v in e.items():
        ref = g["embeddings"][k]
        assert (len(v) == 0 and len(ref) == 0) or (v.dtype == np.float64 and np.array_equal(v, ref.numpy())), k


def test_trajectory_values_are_minus_one_for_a_single_prediction():
    from mcvd_pytorch_amd import metrics
    fake, real = fvd_ref.make_features(5, 16, 12, 12)
    out = metrics.summarize_fvd(fake, real, 1, "2", distance_cpu)
    assert list(out) == ["fvd2", "fvd2_traj_mean", "fvd2_traj_std", "fvd2_traj_conf95"]
    assert out["fvd2"] == distance_cpu(fake, real) and [out[k] for k in list(out)[1:]] == [-1, -1, -1]
    out3 = metrics.summarize_fvd(fake, real, 3, "", distance_cpu)
    vals = [distance_cpu(fake, real, t, 3) for t in range(3)]
    assert out3["fvd_traj_mean"] == float(np.mean(vals)) and out3["fvd_traj_std"] == float(np.std(vals))
    import scipy.stats
    lo = scipy.stats.norm.interval(0.95, loc=np.mean(vals), scale=scipy.stats.sem(vals))[0]
    assert abs(out3["fvd_traj_conf95"] - (np.mean(vals) - lo)) <= 1e-12 * abs(np.mean(vals))


def test_trajectories_do_not_touch_numpys_global_rng():
    from mcvd_pytorch_amd import metrics
    fake, real = fvd_ref.make_features(5, 16, 12, 12)
    np.random.seed(3)
    state = np.random.get_state()
    metrics.fvd_stuff(fake, real, 3, distance_cpu)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]


def test_without_a_detector_nothing_changes(golden_dir):
    from mcvd_pytorch_amd import VideoMetrics
    g = runner(golden_dir, "B")
    sig = inspect.signature(VideoMetrics.__init__)
    assert list(sig.parameters) == ["self", "config", "preds_per_test", "scorenet", "lpips", "fvd", "fvd_batch"]
    assert sig.parameters["fvd"].default is None and sig.parameters["fvd_batch"].default == 10
    assert list(inspect.signature(VideoMetrics.update).parameters) == ["self", "pred01", "real01", "phase", "cond01"]
    vm = VideoMetrics(config_of(g), preds_per_test=2)              # sampling.fvd is True in this config: no detector, no FVD
    for ph in (1, 2):
        vm.vid[ph][0].extend([np.float32(0.01), np.float32(0.02), np.float32(0.03), np.float32(0.04)])
        vm.vid[ph][1].extend([0.5, 0.6, 0.7, 0.8])
    keys = ["preds_per_test"] + [f"{m}{s}{t}" for s in ("", "2") for m in ("mse", "psnr", "ssim") for t in ("", "_std", "_conf95")]
    assert list(vm.summary()) == keys
    with pytest.raises(ValueError):
        vm.update_gen(torch.zeros(4, 3, 32, 32))
    with pytest.raises(ValueError):
        vm.embeddings()


def test_a_detector_without_cond_is_refused_before_the_device(golden_dir):
    from mcvd_pytorch_amd import VideoMetrics
    g = runner(golden_dir, "A")
    called = []
    vm = VideoMetrics(config_of(g), preds_per_test=1, fvd=lambda *a, **kw: called.append(1))
    with pytest.raises(ValueError, match="cond01"):
        vm.update(g["pred_1"][0], g["real_1"][0], phase=1)
    assert not called and vm.vid[1] == ([], [])
    with pytest.raises(ValueError):
        VideoMetrics(config_of(g), fvd=lambda *a, **kw: None, fvd_batch=0)
