"""Golden vectors of the FVD path as the REAL reference computes it -- build container only (needs the reference checkout and scipy).

    PYTHONDONTWRITEBYTECODE=1 python -m tools.gen_fvd_golden [direct A B C]

Modelled on tools/gen_lpips_golden.py and tools/gen_video_metrics_golden.py.  The real `preprocess_single`, `frechet_distance` and
`NCSNRunner.video_gen` (with `sampling.fvd = True`) run.  Replaced from the outside, nothing else:
  * `load_i3d_pretrained` -> tests/fvd_ref.py's StandInDetector(SEED): the I3D is a TorchScript file that is not here (and is fetched with
    wget where it is missing, models/fvd/fvd.py:32-38); what is compared is the path around the detector, which does not depend on which
    detector runs.  Only the seed is stored;
  * `get_fvd_feats` -> get_feats (models/fvd/fvd.py:41-49) restated around the REAL preprocess_single: its line :45 moves everything to
    "cuda:0" whenever `device is not torch.device("cpu")`, an identity test that is always true, so it cannot run here as written.  The
    restated four lines: feats = np.empty((0, 400)); for each batch of bs = 10 videos: np.vstack([feats, detector(torch.stack(
    [preprocess_single(v) for v in batch]), rescale=False, resize=False, return_features=True).detach().cpu().numpy()]);
  * as tools/gen_video_metrics_golden.py: `get_dataset` (in-memory clips), `ssim` (0.0) and `eval_models.PerceptualLoss` (a zero distance)
    -- those metrics are not part of these fixtures --, `st` (scipy.stats with norm.interval(alpha=) mapped to scipy 1.15's `confidence`),
    the plot helpers, and `get_proc_mem` as the cut right after the format_p line, where video_gen's locals are read.
Nothing is written when `ref_abs_dev` exceeds 1e-6 (a sanity cap that separates fp32 rounding from a wrong coordinate rule, not a tolerance).

tests/golden/fvd_direct.pt:
    seed, probe_n, resize [{S, channels, frame_seed, B, T, sum, probe_seed, values, ref_abs_dev, unfused_abs_dev}] -- seeded frames
    (fvd_ref.make_frames), the fp64 sum and probes (fvd_ref.probe_index) of the REAL preprocess_single of the to_i3d clips, and the maximum
    absolute difference of the real output from fvd_ref.preprocess64 (and from the unfused coordinate rule, for the record);
    ref_abs_dev (the maximum over the cases); features [{name, seed, d, n_fake, n_real, start, step, full_rank, value, fake_probe,
    real_probe}] -- fvd_ref.make_features sets with the REAL frechet_distance(fake[start::step], real) on float64 arrays;
    feature_recipe, detector_recipe.
tests/golden/fvd_runner_<case>.pt (real video_gen runs on the tiny nets):
    config_name, overrides, channels, preds_per_test, nfp, batch, iters, seed (of the stand-in), gates (self.calc_fvd1/2/3), second_calc,
    pred_1 / real_1 / cond_1 [iters, B, ...] (what inverse_data_transform returned in phase (1)), pred_2 / real_2 / cond_2, pred_3 (the
    unconditional prediction), calls [(kind, rows) per get_fvd_feats call], call_feats [the features each call returned],
    embeddings {the six arrays of video_embeddings_{ckpt}.npz, float64; [] where not computed}, vid_metrics (the runner's dict),
    fvd_keys (its fvd* keys in order), feat_dev (max |detector(real preprocess_single clips) - detector(fp32(preprocess64 clips))|).
"""
import argparse
import contextlib
import io
import logging
import os
import sys
import tempfile
from unittest import mock

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import scipy.stats  # noqa: E402
import torch  # noqa: E402

from oracle import synth  # noqa: E402
from oracle.gen_runner_golden import import_real_runner, runner_config  # noqa: E402
from tests import fvd_ref  # noqa: E402
from tools.gen_video_tasks_golden import OUT, _save  # noqa: E402

SEED = 11
CAP = 1e-6
PROBE_N = 2048
SIZES = (11, 48, 64, 128, 256, 300)
FEATURES = (
    dict(name="d16_40_24", seed=101, d=16, n_fake=40, n_real=24, full_rank=True),
    dict(name="d400_1024_512", seed=102, d=400, n_fake=1024, n_real=512, full_rank=True),
    dict(name="d16_12_12", seed=103, d=16, n_fake=12, n_real=12, full_rank=False),
    dict(name="d400_256_256", seed=104, d=400, n_fake=256, n_real=256, full_rank=False),
    dict(name="d400_64_32", seed=105, d=400, n_fake=64, n_real=32, full_rank=False),
    dict(name="d400_20_10", seed=106, d=400, n_fake=20, n_real=10, full_rank=False),
    dict(name="d400_96_40_strided", seed=107, d=400, n_fake=96, n_real=40, start=1, step=3, full_rank=False),
)
CASES = {
    # (1) prediction only: tiny (C = 1, 2 cond + 2 frames per block), 8 frames predicted (2 + 8 >= 10), preds_per_test 1
    "A": dict(name="tiny", nfp=8, batch=3, ppt=1, n_clips=6, iters=2),
    # (1) interpolation + (2) prediction: tiny_spade (C = 3, 1 cond + 1 future) with 8 frames per block (1 + 8 + 1 >= 10), 9 predicted
    "B": dict(name="tiny_spade", nfp=9, batch=4, ppt=2, n_clips=2, iters=1, data=dict(num_frames=8, prob_mask_future=0.5)),
    # (1) prediction + (3) generation: tiny with prob_mask_cond, preds_per_test 2
    "C": dict(name="tiny", nfp=8, batch=4, ppt=2, n_clips=4, iters=2, data=dict(prob_mask_cond=0.5)),
}


class _Cut(Exception):
    pass


def gen_direct():
    R = import_real_runner()
    import models.fvd.fvd as real_fvd
    out = dict(seed=SEED, probe_n=PROBE_N, resize=[], features=[], feature_recipe=fvd_ref.FEATURE_RECIPE,
               detector_recipe=fvd_ref.DETECTOR_RECIPE)
    assert R.frechet_distance is real_fvd.frechet_distance
    for S in SIZES:
        for Cc in (1, 3):
            B, T = 1, 2
            frame_seed, probe_seed = 1000 + 10 * S + Cc, 2000 + 10 * S + Cc
            frames = fvd_ref.make_frames(frame_seed, B, T * Cc, S)
            video = fvd_ref.to_i3d(frames, Cc)                                              # [B, 3, T, S, S]
            real = torch.stack([real_fvd.preprocess_single(v) for v in video])            # the REAL function
            assert real.dtype == torch.float32 and tuple(real.shape) == (B, 3, T, 224, 224)
            dev = (real.double() - fvd_ref.preprocess64(video)).abs().max().item()
            dev_unfused = (real.double() - fvd_ref.preprocess64(video, fvd_ref.axis_table_unfused)).abs().max().item()
            assert dev <= CAP, f"S = {S}: the fp64 restatement is {dev:.3e} away from the real preprocess_single: not the same function"
            s, _, values = fvd_ref.probe(real, PROBE_N, probe_seed)
            out["resize"].append(dict(S=S, channels=Cc, frame_seed=frame_seed, B=B, T=T, sum=s, probe_seed=probe_seed, values=values,
                                      ref_abs_dev=dev, unfused_abs_dev=dev_unfused))
            sys.stdout.write(f"  S {S:3d} C {Cc}: ref_abs_dev {dev:.3e} (unfused rule {dev_unfused:.3e})\n")
    out["ref_abs_dev"] = max(c["ref_abs_dev"] for c in out["resize"])
    for spec in FEATURES:
        fake, real = fvd_ref.make_features(spec["seed"], spec["d"], spec["n_fake"], spec["n_real"])
        start, step = spec.get("start", 0), spec.get("step", 1)
        value = real_fvd.frechet_distance(fake[start::step].double().numpy(), real.double().numpy())        # the REAL function
        assert np.isfinite(value) and value > 0
        out["features"].append(dict(spec, start=start, step=step, value=value, fake_probe=fvd_ref.probe(fake, 64, spec["seed"]),
                                    real_probe=fvd_ref.probe(real, 64, spec["seed"] + 1)))
        sys.stdout.write(f"  {spec['name']}: frechet_distance {value!r}\n")
    _save("fvd_direct", out)
    sys.stdout.write(f"wrote fvd_direct.pt: ref_abs_dev {out['ref_abs_dev']:.3e}\n")


def gen_runner(case, subsample=10):
    spec = CASES[case]
    R = import_real_runner()
    import models.fvd.fvd as real_fvd
    batch, ppt = spec["batch"], spec["ppt"]
    config = runner_config(spec["name"], batch, spec["nfp"], subsample)
    for k, v in spec.get("data", {}).items():
        setattr(config.data, k, v)
    config.sampling.preds_per_test = ppt
    config.sampling.max_data_iter = spec["iters"]
    config.sampling.fvd = True
    d = config.data
    C, nf, nc, S, future = d.channels, d.num_frames, d.num_frames_cond, d.image_size, getattr(d, "num_frames_future", 0)
    second = future > 0 and d.prob_mask_future > 0 and not d.prob_mask_sync
    gen = d.prob_mask_cond > 0 and nc + spec["nfp"] >= 10
    T = nc + max(spec["nfp"], nf) + future
    clips = torch.rand(spec["n_clips"], T, C, S, S, generator=torch.Generator().manual_seed(43))
    ds = torch.utils.data.TensorDataset(clips, torch.zeros(spec["n_clips"]))
    tmp = tempfile.mkdtemp(prefix="mcvd_fvd_")
    args = argparse.Namespace(log_path=tmp, data_path=tmp, start_at=0, image_folder=tmp, video_folder=tmp)
    net = R.get_model(config)
    net.load_state_dict(synth.make_state_dict(config, seed=123), strict=False)
    net.eval()
    runner = R.NCSNRunner(args, config, None)
    detector = fvd_ref.StandInDetector(SEED).eval()

    roles = [("real", 1), ("cond", 1), ("pred", 1)] + ([("real", 2), ("cond", 2), ("pred", 2)] if second else []) + ([("pred", 3)] if gen else [])
    rec = {f"{r}_{p}": [] for r, p in roles}
    n_idt = [0]
    calls, call_feats, devs = [], [], []
    real_idt = R.inverse_data_transform

    def inverse_data_transform(cfg, X):
        role, ph = roles[n_idt[0] % len(roles)]
        n_idt[0] += 1
        out = real_idt(cfg, X)
        rec[f"{role}_{ph}"].append(out.clone())
        return out

    def get_fvd_feats(videos, i3d, device, bs=10):
        assert i3d is detector
        kw = dict(rescale=False, resize=False, return_features=True)
        feats = np.empty((0, 400))                                                         # models/fvd/fvd.py:44
        for i in range((len(videos) - 1) // bs + 1):                                       # :47
            x = torch.stack([real_fvd.preprocess_single(video) for video in videos[i * bs:(i + 1) * bs]])     # :48, the REAL function
            feats = np.vstack([feats, i3d(x, **kw).detach().cpu().numpy()])
            x64 = fvd_ref.preprocess64(videos[i * bs:(i + 1) * bs])
            dev_x = (x.double() - x64).abs().max().item()
            assert dev_x <= CAP, dev_x
            devs.append((i3d(x, **kw).double() - i3d(x64.float(), **kw).double()).abs().max().item())
        calls.append((tuple(videos.shape), len(videos)))
        call_feats.append(torch.from_numpy(feats.copy()))
        return feats

    class _Norm:
        @staticmethod
        def interval(alpha, loc=0.0, scale=1.0):
            return scipy.stats.norm.interval(alpha, loc=loc, scale=scale)

    class _St:
        norm = _Norm()
        sem = staticmethod(scipy.stats.sem)

    class _Lpips:
        def forward(self, a, b):
            return torch.zeros(1)

    grabbed = {}
    names = ("vid_metrics", "real_embeddings", "fake_embeddings", "real_embeddings2", "fake_embeddings2", "real_embeddings_uncond",
             "fake_embeddings_uncond")

    def get_proc_mem():
        f = sys._getframe(1).f_locals
        for k in names:
            grabbed[k] = f.get(k)
        raise _Cut()

    log = io.StringIO()
    handler = logging.StreamHandler(log)
    root = logging.getLogger()
    root.addHandler(handler)
    root.setLevel(logging.INFO)
    torch.manual_seed(1234)
    np_state = np.random.get_state()
    try:
        with contextlib.redirect_stdout(io.StringIO()), \
                mock.patch.object(R, "get_dataset", lambda *a, **kw: (ds, ds)), \
                mock.patch.object(R.eval_models, "PerceptualLoss", lambda *a, **kw: _Lpips()), \
                mock.patch.object(R, "ssim", lambda *a, **kw: 0.0), mock.patch.object(R, "st", _St()), \
                mock.patch.object(R, "load_i3d_pretrained", lambda *a, **kw: detector), \
                mock.patch.object(R, "get_fvd_feats", get_fvd_feats), \
                mock.patch.object(R, "putText", lambda f, *a, **kw: f), \
                mock.patch.object(R, "make_grid", lambda *a, **kw: torch.zeros(3, 8, 8)), \
                mock.patch.object(R, "save_image", lambda *a, **kw: None), \
                mock.patch.object(R, "get_proc_mem", get_proc_mem), \
                mock.patch.object(R, "inverse_data_transform", inverse_data_transform):
            try:
                runner.video_gen(scorenet=net, ckpt=0, train=False)
                raise RuntimeError("video_gen returned before its format_p line")
            except _Cut:
                pass
    finally:
        root.removeHandler(handler)
        np.random.set_state(np_state)
    assert n_idt[0] == len(roles) * spec["iters"], (n_idt[0], roles)
    vm = grabbed["vid_metrics"]
    gates = (bool(runner.calc_fvd1), bool(runner.calc_fvd2), bool(runner.calc_fvd3))
    assert any(gates) and gates[2] == gen, gates
    emb = {}
    for k, name in zip(names[1:], ("real_embeddings", "fake_embeddings", "real_embeddings2", "fake_embeddings2", "real_embeddings3",
                                   "fake_embeddings3")):
        v = grabbed[k]
        emb[name] = torch.from_numpy(np.asarray(v, dtype=np.float64).copy()) if len(v) and isinstance(v, np.ndarray) else []
        assert isinstance(v, np.ndarray) or len(v) == 0, (k, type(v))
    out = dict(case=case, config_name=spec["name"], overrides=dict(spec.get("data", {})), channels=C, preds_per_test=ppt, nfp=spec["nfp"],
               batch=batch, iters=spec["iters"], subsample=subsample, seed=SEED, detector_recipe=fvd_ref.DETECTOR_RECIPE, gates=gates,
               second_calc=bool(second), calls=calls, call_feats=call_feats, embeddings=emb,
               vid_metrics={k: (float(v) if isinstance(v, (float, np.floating)) else v) for k, v in vm.items()},
               fvd_keys=[k for k in vm if k.startswith("fvd")], feat_dev=max(devs))
    for k, v in rec.items():
        out[k] = torch.stack(v)
    tag = f"fvd_runner_{case}"
    _save(tag, out)
    sys.stdout.write(f"wrote {tag}.pt: gates {gates}, {len(calls)} detector calls {[n for _, n in calls]}, feat_dev {out['feat_dev']:.3e}\n"
                     f"  {({k: out['vid_metrics'][k] for k in out['fvd_keys']})}\n")


if __name__ == "__main__":
    torch.set_num_threads(4)
    for c in sys.argv[1:] or ["direct", "A", "B", "C"]:
        gen_direct() if c == "direct" else gen_runner(c)
