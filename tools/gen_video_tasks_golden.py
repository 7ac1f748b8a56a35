"""Golden vectors of the three phases of the REAL `NCSNRunner.video_gen` -- build container only (needs the reference checkout).

    PYTHONDONTWRITEBYTECODE=1 python -m tools.gen_video_tasks_golden [A B C D E F]

Reuses oracle/gen_runner_golden.py (`import_real_runner`: the real module with stand-ins for the absent third-party packages;
`runner_config`) and drives the real `video_gen` (runners/ncsn_runner.py:1304-1916) through (1) prediction / interpolation, (2)
prediction with the future block masked and (3) unconditional generation, on the CPU.  Replaced from the outside only: `get_dataset`
(in-memory clips), `load_i3d_pretrained` / `get_fvd_feats` / `frechet_distance` (phase (3) runs under `sampling.fvd` only), `ssim`
(0.0) and `eval_models.PerceptualLoss` (a zero distance): the run goes through the metric code of each phase and the metric values
are not part of the fixture.  The run is cut where the last phase's frames reach `inverse_data_transform` (:1570, :1738, :1916).

A spy on the bound sampler records every call: phase, block, x_init, cond, cond_mask (cloned: phase (3) fills it with ones in place
after block 0, :1885-1886), the keyword arguments, the injected step noise, the output frames and the `verbose` lines.

Fixture tests/golden/tiny_runner_task_<case>.pt (tensors larger than 256 KB live in companion files, see tests/golden_io.py):
    clips, order (dataset rows served), cf [(real, cond, cond_mask) per conditioning_fn call], phases [(task, num_frames_pred)],
    call_phase / call_block / call_kwargs / call_cond_mask / call_log_lines (one entry per sampler call that returned),
    x_init [calls, B, C*nf, S, S], call_cond [calls, B, C*(nc+future), S, S], call_out [calls, B, C*nf, S, S],
    step_noise [calls, subsample - 1, B, C*nf, S, S], pred_raw {task: frames before inverse_data_transform},
    error (case F: {type, phase, block, cond_channels}) or None.
"""
import argparse
import contextlib
import io
import math
import os
import sys
import tempfile
from unittest import mock

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import torch  # noqa: E402

from oracle import synth  # noqa: E402
from oracle.gen_runner_golden import ABSENT, OUT, import_real_runner, runner_config  # noqa: E402

CASES = {
    # tiny + one future frame (concat stem): (1) interpolation, one block
    "A": dict(name="tiny", nfp=2, data=dict(num_frames_future=1)),
    # tiny_spade (nc 1, future 1, nf 2): (1) interpolation + (2) three blocks with the zero future block kept, SPADE cond
    "B": dict(name="tiny_spade", nfp=5, data=dict(prob_mask_future=0.5)),
    # cond_emb net, preds_per_test 2: (1) prediction, 4 blocks + (3) generation of 10 frames, 5 blocks
    "C": dict(name="tiny", nfp=8, data=dict(prob_mask_cond=0.5), model=dict(cond_emb=True), sampling=dict(preds_per_test=2)),
    # all three phases, (3) with the future block
    "D": dict(name="tiny", nfp=8, data=dict(num_frames_future=1, prob_mask_cond=0.5, prob_mask_future=0.5)),
    # D with prob_mask_sync: (1) + (3)
    "E": dict(name="tiny", nfp=8, data=dict(num_frames_future=1, prob_mask_cond=0.5, prob_mask_future=0.5, prob_mask_sync=True)),
    # B under one_frame_at_a_time: (1) as two one-frame blocks, then the reference's failure at the second block of (2)
    "F": dict(name="tiny_spade", nfp=5, data=dict(prob_mask_future=0.5), sampling=dict(one_frame_at_a_time=True)),
}
SPLIT_BYTES = 256 << 10         # tensors above this go to companion files
PART_BYTES = 900 << 10          # each companion file stays below 1 MiB
MAIN_BYTES = 800 << 10          # tensors left in the main file


class _Cut(Exception):
    pass


def _phase_of(future, p_cond, p_future):
    return {(0.0, 0.0): "interp" if future > 0 else "pred", (0.0, 1.0): "pred_future_masked", (1.0, 1.0): "gen"}[(p_cond, p_future)]


def _expected_phases(config):
    """The runner's own gates (:1444, :1612, :1783 with calc_fvd3 of :1313-1335), independent of the library's video_tasks."""
    d, s = config.data, config.sampling
    future = getattr(d, "num_frames_future", 0)
    ph = ["interp" if future > 0 else "pred"]
    if future > 0 and d.prob_mask_future > 0 and not d.prob_mask_sync:
        ph.append("pred_future_masked")
    if d.prob_mask_cond > 0 and d.num_frames_cond + s.num_frames_pred >= 10:
        ph.append("gen")
    return ph


def gen_case(case, batch=2, subsample=10, n_clips=4):
    spec = CASES[case]
    R = import_real_runner()
    import models as ref_models
    config = runner_config(spec["name"], batch, spec["nfp"], subsample)
    for sect in ("data", "model", "sampling"):
        for k, v in spec.get(sect, {}).items():
            setattr(getattr(config, sect), k, v)
    config.sampling.fvd = True
    d = config.data
    C, nf, nc, S, future = d.channels, d.num_frames, d.num_frames_cond, d.image_size, getattr(d, "num_frames_future", 0)
    phases = _expected_phases(config)
    T = nc + max(spec["nfp"], nf) + future
    g = torch.Generator().manual_seed(31)
    clips = torch.rand(n_clips, T, C, S, S, generator=g)
    ds = torch.utils.data.TensorDataset(clips, torch.zeros(n_clips))
    tmp = tempfile.mkdtemp(prefix="mcvd_tasks_")
    args = argparse.Namespace(log_path=tmp, data_path=tmp, start_at=0, image_folder=tmp, video_folder=tmp)

    net = R.get_model(config)
    net.load_state_dict(synth.make_state_dict(config, seed=123), strict=False)
    net.eval()
    runner = R.NCSNRunner(args, config, None)

    per_call = subsample - 1                                                   # DDPM step draws of one call (t_min <= 0)
    n_calls_max = 32
    step_noise = torch.randn(n_calls_max, per_call, batch, C * nf, S, S, generator=torch.Generator().manual_seed(77))
    st = dict(phase=None, block=0, call=-1, draw=0, real_t=None)
    cf, calls = [], []
    printed = io.StringIO()

    def randn_like(like, *a, **kw):
        z = step_noise[st["call"], st["draw"]].to(like)
        st["draw"] += 1
        assert z.shape == like.shape
        return z

    real_dt, real_cf, real_idt = R.data_transform, R.conditioning_fn, R.inverse_data_transform

    def data_transform(cfg, X):
        out = real_dt(cfg, X)
        st["real_t"] = out.clone()
        return out

    def conditioning_fn(cfg, X, num_frames_pred=0, prob_mask_cond=0.0, prob_mask_future=0.0, conditional=True):
        out = real_cf(cfg, X, num_frames_pred=num_frames_pred, prob_mask_cond=prob_mask_cond, prob_mask_future=prob_mask_future,
                      conditional=conditional)
        st["phase"], st["block"] = _phase_of(future, prob_mask_cond, prob_mask_future), 0
        cf.append(dict(phase=st["phase"], num_frames_pred=num_frames_pred, out=tuple(None if t is None else t.clone() for t in out)))
        return out

    roles = ["real", "cond", "pred"] + (["real", "cond", "pred"] if "pred_future_masked" in phases else []) + \
        (["pred"] if "gen" in phases else [])
    preds, n_idt = {}, [0]

    def inverse_data_transform(cfg, X):
        role = roles[n_idt[0]]
        n_idt[0] += 1
        if role == "pred":
            preds[st["phase"]] = X.clone()
            if n_idt[0] == len(roles):
                raise _Cut()
        return real_idt(cfg, X)

    real_sampler = ref_models.ddpm_sampler

    def spy_sampler(x_mod, scorenet, **kw):
        rec = dict(phase=st["phase"], block=st["block"], x_init=x_mod.clone(), cond=kw["cond"].clone(),
                   cond_mask=None if kw.get("cond_mask") is None else kw["cond_mask"].clone(),
                   kwargs={k: v for k, v in kw.items() if k not in ("cond", "cond_mask", "config")})
        st["block"] += 1
        st["call"], st["draw"] = st["call"] + 1, 0
        calls.append(rec)
        mark = len(printed.getvalue())
        out = real_sampler(x_mod, scorenet, **kw)                               # the failure of case F propagates from here
        assert st["draw"] == per_call, st["draw"]
        rec["out"] = out[-1].clone()
        rec["log_lines"] = [ln for ln in printed.getvalue()[mark:].splitlines() if ln.startswith("DDPM: ")]
        return out

    class _Lpips:
        def forward(self, a, b):
            return torch.zeros(1)

    error = None
    torch.manual_seed(1234)
    with contextlib.redirect_stdout(printed), mock.patch.object(R, "get_dataset", lambda *a, **kw: (ds, ds)), \
            mock.patch.object(R.eval_models, "PerceptualLoss", lambda *a, **kw: _Lpips()), \
            mock.patch.object(R, "ssim", lambda *a, **kw: 0.0), \
            mock.patch.object(R, "load_i3d_pretrained", lambda *a, **kw: None), \
            mock.patch.object(R, "get_fvd_feats", lambda *a, **kw: torch.zeros(1, 4)), \
            mock.patch.object(R, "frechet_distance", lambda *a, **kw: 0.0), \
            mock.patch.object(R, "data_transform", data_transform), \
            mock.patch.object(R, "conditioning_fn", conditioning_fn), \
            mock.patch.object(R, "inverse_data_transform", inverse_data_transform), \
            mock.patch.object(R, "ddpm_sampler", spy_sampler), \
            mock.patch.object(torch, "randn_like", randn_like):
        try:
            runner.video_gen(scorenet=net, ckpt=0, train=False)
            raise RuntimeError("video_gen returned before the last phase's frames")
        except _Cut:
            pass
        except RuntimeError as e:
            if "out" in calls[-1]:
                raise
            bad = calls.pop()
            error = dict(type=type(e).__name__, phase=bad["phase"], block=bad["block"], cond_channels=int(bad["cond"].shape[1]),
                         message=str(e).splitlines()[0])
    assert calls and len(calls) <= n_calls_max
    real_t = st["real_t"]
    order = [int(((real_dt(config, clips) - real_t[r]).flatten(1).abs().max(dim=1).values).argmin()) for r in range(batch)]
    n = len(calls)
    out = dict(case=case, config_name=spec["name"], overrides={k: dict(spec.get(k, {})) for k in ("data", "model", "sampling")},
               batch=batch, nfp=spec["nfp"], subsample=subsample, clips=clips, order=order, cf=cf,
               phases=[(p, next(c["num_frames_pred"] for c in cf if c["phase"] == p)) for p in phases if any(c["phase"] == p for c in cf)],
               call_phase=[c["phase"] for c in calls], call_block=[c["block"] for c in calls], call_kwargs=[c["kwargs"] for c in calls],
               call_cond_mask=[c["cond_mask"] for c in calls], call_log_lines=[c["log_lines"] for c in calls],
               x_init=torch.stack([c["x_init"] for c in calls]), call_cond=torch.stack([c["cond"] for c in calls]),
               call_out=torch.stack([c["out"] for c in calls]), step_noise=step_noise[:n].clone(), pred_raw=preds, error=error,
               stood_in=sorted(ABSENT))
    tag = f"tiny_runner_task_{case}"
    _save(tag, out)
    sys.stdout.write(f"wrote {tag}.pt: phases {out['phases']}, {n} sampler calls {list(zip(out['call_phase'], out['call_block']))}, "
                     f"rows {order}, error {error}\n")


def _nbytes(v):
    if torch.is_tensor(v):
        return v.numel() * v.element_size()
    if isinstance(v, dict):
        return sum(_nbytes(x) for x in v.values())
    if isinstance(v, (list, tuple)):
        return sum(_nbytes(x) for x in v)
    return 0


def _save(tag, out):
    """Top-level tensors go to companion files, largest first, while they are above SPLIT_BYTES or the main file would be near 1 MiB."""
    for k in sorted((k for k in out if torch.is_tensor(out[k])), key=lambda k: -_nbytes(out[k])):
        v = out[k]
        if _nbytes(v) > SPLIT_BYTES or _nbytes(out) > MAIN_BYTES:
            per = max(1, PART_BYTES // (v[0].numel() * v.element_size()))
            names = []
            for i in range(math.ceil(len(v) / per)):
                names.append(f"{tag}.{k}.{i}.pt")
                torch.save(v[i * per:(i + 1) * per].clone(), os.path.join(OUT, names[-1]))
            out[k] = {"parts": names, "dim": 0}
    path = os.path.join(OUT, f"{tag}.pt")
    torch.save(out, path)
    assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))


if __name__ == "__main__":
    torch.set_num_threads(2)
    os.makedirs(OUT, exist_ok=True)
    for c in sys.argv[1:] or sorted(CASES):
        gen_case(c)
