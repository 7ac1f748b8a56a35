"""Golden vectors of the REAL `NCSNRunner.video_gen(train=False)` driven to its return -- build container only (needs the reference
checkout, scipy and Pillow).

    PYTHONDONTWRITEBYTECODE=1 python -m tools.gen_video_gen_mode_golden [gen interp beyond]

Reuses oracle/gen_runner_golden.py (`import_real_runner`, `runner_config`), the sampler spy of tools/gen_video_tasks_golden.py (a closure
there, restated here record for record, with its `_save`), the metric stand-ins of tools/gen_video_metrics_golden.py (`ssim_scipy`,
`_ToPILImage`; its `st` stand-in is a closure and is restated) and the seeded stand-in detector of tools/gen_fvd_golden.py
(tests/fvd_ref.StandInDetector(SEED) behind get_feats restated around the REAL preprocess_single).  LPIPS is a zero distance, as there.
The whole of runners/ncsn_runner.py:1304-2368 runs on the CPU: the loop over the DataLoader with its `max_data_iter` cut, every phase,
the metric code, the save section, the summary, the alias table and write_to_yaml.  Inert: `get_proc_mem`, the plot helpers (`putText`,
`make_grid`, `save_image`; imageio and cv2 are stand-in modules).  torch.save, np.savez and write_to_yaml write into a scratch folder, which
is read back.

The step noise of sampler call k is torch.randn(subsample - 1, B, C * nf, S, S, generator=torch.Generator().manual_seed(NOISE_SEED + k))
(`step_noise`): the fixture keeps the recipe and the fp64 sum of every call's noise, not the tensors.

Fixture tests/golden/video_gen_mode_<case>.pt (tensors larger than 256 KB live in companion files, see tests/golden_io.py):
    config_name, overrides, batch (sampling.batch_size), preds_per_test, nfp, subsample, max_data_iter, n_batches (the loader's length),
    seed (of the stand-in detector), gates, second_calc,
    served [iters, clips, T, C, S, S]      the clips of every batch the loop ran, before repeat_interleave (what `batches` yields)
    call_batch / call_phase / call_block / call_kwargs / call_cond_mask, x_init, call_cond, call_out   one entry per sampler call
    noise_seed, noise_sums                 the step-noise recipe above and its per-call fp64 sums
    pred_1 / real_1 / cond_1 [iters, B, ...], pred_2 / real_2 / cond_2, pred_3     what each phase handed to its metric code
    vid_mse / vid_mse2 (fp32 arrays or None), vid_mse64 {1: ..., 2: ...}, vid_ssim / vid_ssim2     the runner's per-video lists
    embeddings {the six arrays of video_embeddings_{ckpt}.npz} or None, feat_dev
    returned (the dict handed to write_to_yaml; None where video_gen returned at :2192), returned_keys (its key order),
    yaml (the text of vid_metrics.yml or None), format_p (the "elapsed: ..." lines), saved {file name: {key: shape}}, files (all written)
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
from oracle.gen_runner_golden import ABSENT, import_real_runner, runner_config  # noqa: E402
from tests import fvd_ref  # noqa: E402
from tools.gen_fvd_golden import CAP, SEED  # noqa: E402
from tools.gen_video_metrics_golden import _ToPILImage, ssim_scipy  # noqa: E402
from tools.gen_video_tasks_golden import _phase_of, _save  # noqa: E402

NOISE_SEED = 7700
CASES = {
    # (1) prediction + (3) generation: preds_per_test 2, two of the loader's three batches of two clips
    "gen": dict(name="tiny", nfp=8, batch=4, ppt=2, n_clips=6, iters=2, fvd=True, data=dict(prob_mask_cond=0.5)),
    # (1) interpolation + (2) prediction with the future block masked (tiny_spade: 1 cond + 1 future frame, 2 frames per block)
    "interp": dict(name="tiny_spade", nfp=5, batch=2, ppt=1, n_clips=2, iters=1, fvd=False, data=dict(num_frames_future=1, prob_mask_future=0.5)),
    # sampling.num_frames_pred beyond the clip length: phase (1) cannot calculate and video_gen returns None (:2192)
    "beyond": dict(name="tiny", nfp=4, batch=2, ppt=1, n_clips=2, iters=1, fvd=False, short=True),
}


def step_noise(call, per_call, shape):
    return torch.randn(per_call, *shape, generator=torch.Generator().manual_seed(NOISE_SEED + call))


def gen_case(case, subsample=10):
    spec = CASES[case]
    R = import_real_runner()
    import models as ref_models
    import models.fvd.fvd as real_fvd
    batch, ppt = spec["batch"], spec["ppt"]
    config = runner_config(spec["name"], batch, spec["nfp"], subsample)
    for k, v in spec.get("data", {}).items():
        setattr(config.data, k, v)
    config.sampling.preds_per_test = ppt
    config.sampling.max_data_iter = spec["iters"]
    config.sampling.fvd = spec["fvd"]
    d = config.data
    C, nf, nc, S, future = d.channels, d.num_frames, d.num_frames_cond, d.image_size, getattr(d, "num_frames_future", 0)
    second = bool(future > 0 and d.prob_mask_future > 0 and not d.prob_mask_sync)
    gen = bool(spec["fvd"] and d.prob_mask_cond > 0 and nc + spec["nfp"] >= 10)
    T = nc + (nf if spec.get("short") else max(spec["nfp"], nf)) + future
    clips = torch.rand(spec["n_clips"], T, C, S, S, generator=torch.Generator().manual_seed(47))
    ds = torch.utils.data.TensorDataset(clips, torch.zeros(spec["n_clips"]))
    tmp = tempfile.mkdtemp(prefix="mcvd_mode_")
    args = argparse.Namespace(log_path=tmp, data_path=tmp, start_at=0, image_folder=tmp, video_folder=tmp)
    net = R.get_model(config)
    net.load_state_dict(synth.make_state_dict(config, seed=123), strict=False)
    net.eval()
    runner = R.NCSNRunner(args, config, None)
    detector = fvd_ref.StandInDetector(SEED).eval()

    per_call = subsample - 1
    st = dict(phase=None, block=0, call=-1, draw=0, noise=None, batch=-1)
    calls, served, devs, sums = [], [], [], []
    roles = [("real", 1), ("cond", 1), ("pred", 1)] + ([("real", 2), ("cond", 2), ("pred", 2)] if second else []) + ([("pred", 3)] if gen else [])
    rec = {f"{r}_{p}": [] for r, p in roles}
    n_idt = [0]
    real_dt, real_cf, real_idt = R.data_transform, R.conditioning_fn, R.inverse_data_transform

    def randn_like(like, *a, **kw):
        z = st["noise"][st["draw"]].to(like)
        st["draw"] += 1
        assert z.shape == like.shape
        return z

    def data_transform(cfg, X):
        served.append(X[::ppt].clone())
        st["batch"] += 1
        return real_dt(cfg, X)

    def conditioning_fn(cfg, X, num_frames_pred=0, prob_mask_cond=0.0, prob_mask_future=0.0, conditional=True):
        st["phase"], st["block"] = _phase_of(future, prob_mask_cond, prob_mask_future), 0
        return real_cf(cfg, X, num_frames_pred=num_frames_pred, prob_mask_cond=prob_mask_cond, prob_mask_future=prob_mask_future,
                       conditional=conditional)

    def inverse_data_transform(cfg, X):
        role, ph = roles[n_idt[0] % len(roles)]
        n_idt[0] += 1
        out = real_idt(cfg, X)
        rec[f"{role}_{ph}"].append(out.clone())
        return out

    real_sampler = ref_models.ddpm_sampler

    def spy_sampler(x_mod, scorenet, **kw):
        r = dict(batch=st["batch"], phase=st["phase"], block=st["block"], x_init=x_mod.clone(), cond=kw["cond"].clone(),
                 cond_mask=None if kw.get("cond_mask") is None else kw["cond_mask"].clone(),
                 kwargs={k: v for k, v in kw.items() if k not in ("cond", "cond_mask", "config")})
        st["block"] += 1
        st["call"], st["draw"] = st["call"] + 1, 0
        st["noise"] = step_noise(st["call"], per_call, tuple(x_mod.shape))
        sums.append(float(st["noise"].double().sum()))
        calls.append(r)
        out = real_sampler(x_mod, scorenet, **kw)
        assert st["draw"] == per_call, st["draw"]
        r["out"] = out[-1].clone()
        return out

    def get_fvd_feats(videos, i3d, device, bs=10):
        assert i3d is detector
        kw = dict(rescale=False, resize=False, return_features=True)
        feats = np.empty((0, 400))                                                         # models/fvd/fvd.py:44
        for i in range((len(videos) - 1) // bs + 1):                                       # :47
            x = torch.stack([real_fvd.preprocess_single(video) for video in videos[i * bs:(i + 1) * bs]])     # :48, the REAL function
            feats = np.vstack([feats, i3d(x, **kw).detach().cpu().numpy()])
            x64 = fvd_ref.preprocess64(videos[i * bs:(i + 1) * bs])
            assert (x.double() - x64).abs().max().item() <= CAP
            devs.append((i3d(x, **kw).double() - i3d(x64.float(), **kw).double()).abs().max().item())
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

    grabbed, written = {}, {}
    real_yaml = R.NCSNRunner.write_to_yaml

    def write_to_yaml(self, yaml_file, my_dict):
        written["dict"] = dict(my_dict)
        return real_yaml(self, yaml_file, my_dict)

    def on_return(frame, event, arg):
        if event == "return" and frame.f_code.co_name == "video_gen":
            for k in ("vid_mse", "vid_ssim", "vid_mse2", "vid_ssim2"):
                grabbed[k] = frame.f_locals.get(k)

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
                mock.patch.object(R, "ssim", ssim_scipy), mock.patch.object(R.Transforms, "ToPILImage", _ToPILImage), \
                mock.patch.object(R, "st", _St()), \
                mock.patch.object(R, "load_i3d_pretrained", lambda *a, **kw: detector), \
                mock.patch.object(R, "get_fvd_feats", get_fvd_feats), \
                mock.patch.object(R, "putText", lambda f, *a, **kw: f), \
                mock.patch.object(R, "make_grid", lambda *a, **kw: torch.zeros(3, 8, 8)), \
                mock.patch.object(R, "save_image", lambda *a, **kw: None), \
                mock.patch.object(R, "get_proc_mem", lambda: 0.0), \
                mock.patch.object(R.NCSNRunner, "write_to_yaml", write_to_yaml), \
                mock.patch.object(R, "data_transform", data_transform), \
                mock.patch.object(R, "conditioning_fn", conditioning_fn), \
                mock.patch.object(R, "inverse_data_transform", inverse_data_transform), \
                mock.patch.object(R, "ddpm_sampler", spy_sampler), \
                mock.patch.object(torch, "randn_like", randn_like):
            try:
                sys.setprofile(on_return)
                ret = runner.video_gen(scorenet=net, ckpt=0, train=False)
            finally:
                sys.setprofile(None)
    finally:
        root.removeHandler(handler)
        np.random.set_state(np_state)
    assert ret is None                                      # train=False: the dict goes to write_to_yaml, or None is returned at :2192
    assert len(served) == spec["iters"] and n_idt[0] == len(roles) * spec["iters"], (len(served), n_idt[0])
    returned = written.get("dict")
    files = sorted(f for f in os.listdir(tmp) if os.path.isfile(os.path.join(tmp, f)))
    yml = open(os.path.join(tmp, "vid_metrics.yml")).read() if "vid_metrics.yml" in files else None
    saved = {}
    for f in files:
        if f.endswith(".pt"):
            dd = torch.load(os.path.join(tmp, f), weights_only=False)
            saved[f] = {k: tuple(v.shape) for k, v in dd.items()}
    emb = None
    if "video_embeddings_0.npz" in files:
        z = np.load(os.path.join(tmp, "video_embeddings_0.npz"), allow_pickle=True)
        emb = {k: (torch.from_numpy(np.asarray(z[k], dtype=np.float64).copy()) if z[k].ndim == 2 and len(z[k]) else []) for k in z.files}
    fmt = [ln[ln.index("elapsed:"):] for ln in log.getvalue().splitlines() if "preds_per_test:" in ln]

    n = len(calls)
    out = dict(case=case, config_name=spec["name"], overrides=dict(data=dict(spec.get("data", {}))), batch=batch, preds_per_test=ppt,
               nfp=spec["nfp"], subsample=subsample, max_data_iter=spec["iters"], n_batches=-(-spec["n_clips"] // (batch // ppt)),
               fvd=spec["fvd"], seed=SEED, gates=(bool(runner.calc_fvd1), bool(runner.calc_fvd2), bool(runner.calc_fvd3)), second_calc=second,
               served=torch.stack(served), call_batch=[c["batch"] for c in calls], call_phase=[c["phase"] for c in calls],
               call_block=[c["block"] for c in calls], call_kwargs=[c["kwargs"] for c in calls], call_cond_mask=[c["cond_mask"] for c in calls],
               x_init=torch.stack([c["x_init"] for c in calls]), call_cond=torch.stack([c["cond"] for c in calls]),
               call_out=torch.stack([c["out"] for c in calls]), noise_seed=NOISE_SEED, noise_sums=sums, vid_mse64={},
               embeddings=emb, feat_dev=max(devs) if devs else None,
               returned=None if returned is None else {k: (float(v) if isinstance(v, (float, np.floating)) else v) for k, v in returned.items()},
               returned_keys=None if returned is None else list(returned), yaml=yml, format_p=fmt, saved=saved, files=files,
               stood_in=sorted(ABSENT))
    assert out["gates"][2] == gen, out["gates"]
    for k, v in rec.items():
        out[k] = torch.stack(v)
    for ph, key in ((1, ""), (2, "2")):
        lst = grabbed.get("vid_mse" + key) or []
        if lst and not all(isinstance(v, int) for v in lst):
            out["vid_mse" + key] = np.array([float(v) for v in lst], dtype=np.float32)
            out["vid_ssim" + key] = np.array([float(v) for v in grabbed["vid_ssim" + key]], dtype=np.float64)
            pred, real = torch.cat(rec[f"pred_{ph}"]), torch.cat(rec[f"real_{ph}"])
            Tp = pred.shape[1] // C
            dd = (real[:, :C * Tp].float() - pred.float()).double()
            out["vid_mse64"][ph] = ((dd * dd).reshape(len(pred), Tp, -1).mean(-1).sum(-1) / Tp).numpy()
        else:
            out["vid_mse" + key], out["vid_ssim" + key] = None, None
            out["vid_mse" + key + "_list"] = [int(v) for v in lst]
    tag = f"video_gen_mode_{case}"
    _save(tag, out)
    sys.stdout.write(f"wrote {tag}.pt: {n} sampler calls {list(zip(out['call_batch'], out['call_phase'], out['call_block']))}, gates {out['gates']}, "
                     f"files {files}\n  {fmt[-1] if fmt else None}\n")


if __name__ == "__main__":
    torch.set_num_threads(4)
    for c in sys.argv[1:] or sorted(CASES):
        gen_case(c)
