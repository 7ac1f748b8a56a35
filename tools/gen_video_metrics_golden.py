"""Golden vectors of the metric code of the REAL `NCSNRunner.video_gen` (MSE, PSNR, SSIM) -- build container only (needs the reference
checkout, scipy and Pillow).

    PYTHONDONTWRITEBYTECODE=1 python -m tools.gen_video_metrics_golden [smmnist cityscapes beyond]

Modelled on tools/gen_video_tasks_golden.py and reusing oracle/gen_runner_golden.py (`import_real_runner`, `runner_config`).  The real
`video_gen` runs on the CPU THROUGH its metric code (runners/ncsn_runner.py:1580-1609, :1749-1778) and its summary (:2195-2255) up to the
`format_p` log line.  Replaced from the outside, nothing else:
  * `R.ssim` -> skimage's structural_similarity restated over scipy.ndimage.gaussian_filter (skimage is not installed here; skimage
    itself makes that call: sigma 1.5, truncate 3.5, reflect mode; C1 / C2 of data_range 255; cov_norm 1; mean of S over the interior
    cropped by 5).  This restatement could not be compared with skimage itself on this machine;
  * `R.F.mse_loss` -> a recording pass-through of the real F.mse_loss;
  * `R.Transforms.ToPILImage` -> torchvision's float `to_pil_image` restated (pic.mul(255).byte(), CHW -> HWC, mode L / RGB).  The real
    Pillow `convert("RGB")` / `convert("L")` calls then run inside the real runner code;
  * `R.st` -> scipy.stats with `norm.interval(alpha=...)` mapped to scipy 1.15's positional `confidence`; it records the metric arrays
    it is handed (`sem`) and the intervals;
  * `eval_models.PerceptualLoss` -> a zero distance (LPIPS needs pretrained AlexNet weights); FVD off (`sampling.fvd` False);
  * the plot helpers of the save section (`putText`, `make_grid`, `save_image`) -> inert stand-ins; `get_dataset` -> in-memory clips;
  * `get_proc_mem` -> the cut: it is called right after the `format_p` line and reads the runner's `vid_metrics`, `vid_mse`, ... from
    its caller's frame.  When (1) took the "cannot calculate" branch the runner returns None at :2192 instead (no summary, no
    format_p line); the lists are then read from video_gen's frame as it returns.

Fixture tests/golden/video_metrics_<case>.pt (tensors larger than 256 KB live in companion files, see tests/golden_io.py):
    config_name, dataset, channels, preds_per_test, overrides,
    frames {1: [(pred01, real01) per batch], 2: [...]}     the [0, 1] tensors each phase handed to its metric loop
    grey {1: [uint8 [2, B, T, H, W] per batch], 2: ...}    the planes the real code handed to `ssim` (pred, then real)
    mse {1: [fp32 [B, T] per batch], 2: ...}               what F.mse_loss returned per frame
    ssim {1: [fp64 [B, T] per batch], 2: ...}              what the ssim stand-in returned per frame
    vid_mse / vid_ssim / vid_mse2 / vid_ssim2              the runner's lists (vid_mse as float32 arrays, or int zeros)
    vid_mse64 {1: [...], 2: [...]}                         the fp64 value of each per-video MSE expression
    metric_arrays [the arrays handed to image_metric_stuff, in call order], intervals [(lo, hi) per call]
    vid_metrics (the runner's dict, floats at full precision; None where video_gen returned None), format_p (the log line or None),
    cannot (phases that took :1573-1578)
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
import scipy.ndimage  # noqa: E402
import scipy.stats  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from oracle import synth  # noqa: E402
from oracle.gen_runner_golden import import_real_runner, runner_config  # noqa: E402
from tools.gen_video_tasks_golden import _save  # noqa: E402

CASES = {
    # SMMNIST-named (MNIST rule), C = 1, preds_per_test 2, two batches of two clips: (1) prediction, 2 blocks
    "smmnist": dict(name="tiny", nfp=4, batch=4, ppt=2, n_clips=4, iters=2, dataset="StochasticMovingMNIST"),
    # C = 3 (real quantisation and luma), (1) interpolation + (2) prediction with the future block masked, 2 blocks
    "cityscapes": dict(name="tiny_spade", nfp=3, batch=2, ppt=1, n_clips=2, iters=1, dataset="Cityscapes",
                       data=dict(prob_mask_future=0.5)),
    # clips shorter than the prediction: (1) takes the "cannot calculate" branch (:1573-1578)
    "beyond": dict(name="tiny", nfp=4, batch=2, ppt=1, n_clips=2, iters=1, dataset="KTH", short=True),
}


class _Cut(Exception):
    pass


def ssim_scipy(im1, im2, data_range=None, gaussian_weights=False, use_sample_covariance=True, **kw):
    """skimage.metrics.structural_similarity (>= 0.19) for 2-D input with gaussian_weights=True, use_sample_covariance=False."""
    assert gaussian_weights and not use_sample_covariance and data_range == 255 and not kw
    X, Y = im1.astype(np.float64), im2.astype(np.float64)
    filt = lambda a: scipy.ndimage.gaussian_filter(a, sigma=1.5, truncate=3.5)
    ux, uy, uxx, uyy, uxy = (filt(a) for a in (X, Y, X * X, Y * Y, X * Y))
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    S = (A1 * A2) / (B1 * B2)
    return S[5:-5, 5:-5].mean(dtype=np.float64)


class _ToPILImage:
    """torchvision.transforms.ToPILImage() on a float CHW tensor (functional.to_pil_image): pic.mul(255).byte(), HWC, mode L / RGB."""

    def __call__(self, pic):
        assert pic.is_floating_point() and pic.dim() == 3 and pic.shape[0] in (1, 3)
        a = pic.mul(255).byte().permute(1, 2, 0).numpy()
        return Image.fromarray(a[:, :, 0], mode="L") if a.shape[2] == 1 else Image.fromarray(a, mode="RGB")


def gen_case(case, subsample=10, perceptual=None, extra=None, save=True):
    """perceptual / extra / save: hooks of tools/gen_lpips_golden.py -- `perceptual(R)` builds what replaces eval_models.PerceptualLoss
    (default: the zero distance), `extra(R, stack)` enters further patches, save=False returns the fixture dict (with the runner's
    vid_lpips lists) instead of writing it.  The defaults write exactly the fixture described above."""
    spec = CASES[case]
    R = import_real_runner()
    batch, ppt = spec["batch"], spec["ppt"]
    config = runner_config(spec["name"], batch, spec["nfp"], subsample)
    config.data.dataset = spec["dataset"]
    for k, v in spec.get("data", {}).items():
        setattr(config.data, k, v)
    config.sampling.preds_per_test = ppt
    config.sampling.max_data_iter = spec["iters"]
    config.sampling.fvd = False
    d = config.data
    C, nf, nc, S, future = d.channels, d.num_frames, d.num_frames_cond, d.image_size, getattr(d, "num_frames_future", 0)
    T = nc + (nf if spec.get("short") else max(spec["nfp"], nf)) + future
    clips = torch.rand(spec["n_clips"], T, C, S, S, generator=torch.Generator().manual_seed(41))
    ds = torch.utils.data.TensorDataset(clips, torch.zeros(spec["n_clips"]))
    tmp = tempfile.mkdtemp(prefix="mcvd_metrics_")
    args = argparse.Namespace(log_path=tmp, data_path=tmp, start_at=0, image_folder=tmp, video_folder=tmp)
    net = R.get_model(config)
    net.load_state_dict(synth.make_state_dict(config, seed=123), strict=False)
    net.eval()
    runner = R.NCSNRunner(args, config, None)

    st = dict(phase=1)
    rec = dict(frames={1: [], 2: []}, grey={1: [], 2: []}, mse={1: [], 2: []}, ssim={1: [], 2: []}, metric_arrays=[], intervals=[])
    cur = {}
    roles = ["real", "cond", "pred"] * (2 if future > 0 and d.prob_mask_future > 0 else 1)
    n_idt = [0]
    real_cf, real_idt, real_mse = R.conditioning_fn, R.inverse_data_transform, torch.nn.functional.mse_loss

    def conditioning_fn(cfg, X, num_frames_pred=0, prob_mask_cond=0.0, prob_mask_future=0.0, conditional=True):
        st["phase"] = 2 if prob_mask_future == 1.0 else 1
        return real_cf(cfg, X, num_frames_pred=num_frames_pred, prob_mask_cond=prob_mask_cond, prob_mask_future=prob_mask_future,
                       conditional=conditional)

    def inverse_data_transform(cfg, X):
        role = roles[n_idt[0] % len(roles)]
        n_idt[0] += 1
        out = real_idt(cfg, X)
        if role in ("real", "pred"):
            cur[role] = out.clone()
        if role == "pred":
            ph = st["phase"]
            rec["frames"][ph].append((cur["pred"], cur["real"]))
            rec["mse"][ph].append([])
            rec["ssim"][ph].append([])
            rec["grey"][ph].append([])
        return out

    def mse_loss(a, b, *args, **kw):
        out = real_mse(a, b, *args, **kw)
        rec["mse"][st["phase"]][-1].append(out.clone())
        return out

    def ssim(p, r, **kw):
        v = ssim_scipy(p, r, **kw)
        rec["ssim"][st["phase"]][-1].append(v)
        rec["grey"][st["phase"]][-1].append((p.copy(), r.copy()))
        return v

    class _Norm:
        @staticmethod
        def interval(alpha, loc=0.0, scale=1.0):
            out = scipy.stats.norm.interval(alpha, loc=loc, scale=scale)
            rec["intervals"].append(tuple(float(x) for x in out))
            return out

    class _St:
        norm = _Norm()

        @staticmethod
        def sem(metric):
            rec["metric_arrays"].append(np.array(metric, copy=True))
            return scipy.stats.sem(metric)

    class _Lpips:
        def forward(self, a, b):
            return torch.zeros(1)

    grabbed = {}

    def get_proc_mem():
        f = sys._getframe(1).f_locals
        for k in ("vid_metrics", "vid_mse", "vid_ssim", "vid_mse2", "vid_ssim2", "vid_lpips", "vid_lpips2"):
            grabbed[k] = f.get(k)
        raise _Cut()

    def on_return(frame, event, arg):
        # the "cannot calculate" run returns at :2192 before get_proc_mem: its lists are read from video_gen's frame as it returns
        if event == "return" and frame.f_code.co_name == "video_gen":
            for k in ("vid_mse", "vid_ssim", "vid_mse2", "vid_ssim2", "vid_lpips", "vid_lpips2"):
                grabbed[k] = frame.f_locals.get(k)

    log = io.StringIO()
    handler = logging.StreamHandler(log)
    root = logging.getLogger()
    root.addHandler(handler)
    root.setLevel(logging.INFO)
    model_lpips = perceptual(R) if perceptual is not None else _Lpips()      # built before the seed: its construction draws
    torch.manual_seed(1234)
    try:
        with contextlib.ExitStack() as stack, contextlib.redirect_stdout(io.StringIO()), \
                mock.patch.object(R, "get_dataset", lambda *a, **kw: (ds, ds)), \
                mock.patch.object(R.eval_models, "PerceptualLoss", lambda *a, **kw: model_lpips), \
                mock.patch.object(R, "ssim", ssim), mock.patch.object(R.F, "mse_loss", mse_loss), \
                mock.patch.object(R.Transforms, "ToPILImage", _ToPILImage), mock.patch.object(R, "st", _St()), \
                mock.patch.object(R, "putText", lambda f, *a, **kw: f), \
                mock.patch.object(R, "make_grid", lambda *a, **kw: torch.zeros(3, 8, 8)), \
                mock.patch.object(R, "save_image", lambda *a, **kw: None), \
                mock.patch.object(R, "get_proc_mem", get_proc_mem), \
                mock.patch.object(R, "conditioning_fn", conditioning_fn), \
                mock.patch.object(R, "inverse_data_transform", inverse_data_transform):
            if extra is not None:
                extra(R, stack)
            try:
                sys.setprofile(on_return)
                returned = runner.video_gen(scorenet=net, ckpt=0, train=False)
                sys.setprofile(None)
                assert returned is None and rec["frames"][1] and not rec["mse"][1][-1], "video_gen returned before its format_p line"
                grabbed["vid_metrics"] = None                           # :2192: no summary when (1) could not calculate
            except _Cut:
                pass
    finally:
        sys.setprofile(None)
        root.removeHandler(handler)
    fmt = [ln for ln in log.getvalue().splitlines() if "preds_per_test:" in ln]
    assert len(fmt) == (0 if grabbed["vid_metrics"] is None else 1), log.getvalue()

    out = dict(case=case, config_name=spec["name"], dataset=spec["dataset"], channels=C, preds_per_test=ppt,
               overrides=dict(spec.get("data", {})), nfp=spec["nfp"], batch=batch, iters=spec["iters"],
               frames={}, grey={}, mse={}, ssim={}, vid_mse64={}, cannot=[])
    for ph in (1, 2):
        out["frames"][ph] = rec["frames"][ph]
        out["grey"][ph], out["mse"][ph], out["ssim"][ph], out["vid_mse64"][ph] = [], [], [], []
        for bi, (pred, real) in enumerate(rec["frames"][ph]):
            B, Tp = pred.shape[0], pred.shape[1] // C
            if not rec["mse"][ph][bi]:                                  # "cannot calculate": no frame reached the metric loop
                out["cannot"].append(ph)
                continue
            mse = torch.stack(rec["mse"][ph][bi]).reshape(B, Tp)
            out["mse"][ph].append(mse)
            out["ssim"][ph].append(torch.tensor(rec["ssim"][ph][bi], dtype=torch.float64).reshape(B, Tp))
            g = rec["grey"][ph][bi]
            out["grey"][ph].append(torch.stack([torch.from_numpy(np.stack([x[k] for x in g])).reshape(B, Tp, *g[0][0].shape)
                                                for k in (0, 1)]))
            dd = (real[:, :C * Tp].float() - pred.float()).double()
            out["vid_mse64"][ph].append(((dd * dd).reshape(B, Tp, -1).mean(-1).sum(-1) / Tp))
    vm = grabbed["vid_metrics"]
    out["vid_metrics"] = None if vm is None else {k: (float(v) if isinstance(v, (float, np.floating)) else v) for k, v in vm.items()}
    for k in ("vid_mse", "vid_ssim", "vid_mse2", "vid_ssim2"):
        out[k] = np.array(grabbed[k]) if grabbed[k] else None
        out[k + "_list"] = [(int(v) if isinstance(v, int) else float(v)) for v in grabbed[k]]
    out["metric_arrays"], out["intervals"], out["format_p"] = rec["metric_arrays"], rec["intervals"], (fmt or [None])[0]
    if not save:
        for k in ("vid_lpips", "vid_lpips2"):
            out[k + "_list"] = None if grabbed.get(k) is None else [(int(v) if isinstance(v, int) else float(v)) for v in grabbed[k]]
        return out
    tag = f"video_metrics_{case}"
    _save(tag, out)
    sys.stdout.write(f"wrote {tag}.pt: batches {[len(out['frames'][p]) for p in (1, 2)]}, cannot {out['cannot']}\n  {out['format_p']}\n")


if __name__ == "__main__":
    torch.set_num_threads(2)
    for c in sys.argv[1:] or sorted(CASES):
        gen_case(c)
