"""Golden vectors of the REAL `NCSNRunner.sample()` driven from its checkpoint file to its last torch.save -- build container only (needs
the reference checkout).

    PYTHONDONTWRITEBYTECODE=1 python -m tools.gen_sample_mode_golden [final steps uncond_init future fid fid_init]

Reuses oracle/gen_runner_golden.py (`import_real_runner`, `runner_config`) and the `_save` of tools/gen_video_tasks_golden.py.  The whole of
runners/ncsn_runner.py:914-1301 that a case reaches runs on the CPU, unmodified: the checkpoint load with its EMA round trip, the
DataLoader, the transforms and conditioning_fn, the init z, the sampler call, the reshapes, stretch_image, the full row and the saves.
Replaced from the outside only: `get_dataset` (in-memory clips of seeded torch.rand), `data_transform` (a spy that records the served
batch), the bound sampler (a spy that records x_init, cond, cond_mask, the kwargs, the output and the verbose lines of every call),
`torch.randn` (a spy that records the init z), `torch.randn_like` (the step noise recipe below), `make_grid` (records its argument and
nrow), `save_image` (inert); torch.save writes into a scratch folder, which is read back.  The FID cases also replace `get_feats_path`
and `get_fid_PR` -- the latter records gen_samples and returns a fixed triple -- and catch the NameError the reference raises right after
(:1285: `precisions` is never defined in sample()), so nothing is saved there.

Every case writes a real checkpoint.pt / checkpoint_{id}.pt in the reference's list format [model ('module.' keys), optimizer, epoch,
step, EMA shadow], built from oracle/synth.make_state_dict seeds; the fixture keeps the seeds, not the weights.

The step noise of sampler call k is torch.randn(subsample - 1, B, C * nf, S, S, generator=torch.Generator().manual_seed(NOISE_SEED + k))
(`step_noise`): the fixture keeps the recipe and the fp64 sum of every call's noise, not the tensors.

Fixture tests/golden/sample_mode_<case>.pt (tensors larger than 256 KB live in companion files, see tests/golden_io.py):
    config_name, overrides {data, model, sampling}, batch, subsample, sd_seed, ema_seed (None without model.ema), ckpt (the label),
    ckpt_file, fid (bool), n_rounds,
    served [batches, B, T, C, S, S]        every batch that reached data_transform, in order (what the loaders yielded)
    z [calls, B, C*nf, S, S]               the init z of every sampler call
    x_init, call_cond (None for an unconditional net), call_cond_mask, call_has_cond_mask, call_kwargs, call_log_lines
    call_out [calls, (1 | steps), B, C*nf, S, S]     what the sampler returned (a CPU run: step images alias x_mod, see
                                            tests/test_oracle_golden.add_back_step_noise); FID cases: its last image alone
    noise_seed, noise_sums                 the step-noise recipe above and its per-call fp64 sums
    grids [tensor, ...], grid_nrows        what make_grid was handed, in call order
    files, saved {file name: tensor}       the torch.save()s of the run, in order
    gen_samples, fid_triple                FID cases: what get_fid_PR was handed and what the stand-in returned
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile
from unittest import mock

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import torch  # noqa: E402

from oracle import synth  # noqa: E402
from oracle.gen_runner_golden import ABSENT, OUT, import_real_runner, runner_config  # noqa: E402
from tools.gen_video_tasks_golden import _save  # noqa: E402

NOISE_SEED = 9100
SD_SEED, EMA_SEED = 123, 124
FID_TRIPLE = (1.5, 0.25, 0.75)
CASES = {
    # final_only; model.ema with a shadow from a second seed; ckpt_id None -> "latest", checkpoint.pt
    "final": dict(name="tiny", batch=4, model=dict(ema=True, ema_rate=0.999), sampling=dict(final_only=True, ckpt_id=None)),
    # every step image (10 steps + the denoise pass); one frame per block, where :1147's reshape to (B, C, S, S) holds; checkpoint_7.pt
    "steps": dict(name="tiny", batch=3, data=dict(num_frames=1), sampling=dict(final_only=False, ckpt_id=7)),
    # unconditional net started from data: the only unconditional route the reference survives (cond_mask is unbound otherwise, :1135)
    "uncond_init": dict(name="tiny_uncond", batch=3, sampling=dict(final_only=True, data_init=True)),
    # tiny_spade: C = 3, one cond frame + one future frame -> the futr split, the full row with futr, both nrows
    "future": dict(name="tiny_spade", batch=2, sampling=dict(final_only=True)),
    # FID branch, two rounds; the loader holds one batch, so the cond loader starts over
    "fid": dict(name="tiny", batch=3, sampling=dict(fid=True, num_samples4fid=6)),
    # the same from data: cond comes from the init batch (:1244)
    "fid_init": dict(name="tiny", batch=3, sampling=dict(fid=True, num_samples4fid=6, data_init=True)),
}


def step_noise(call, per_call, shape):
    return torch.randn(per_call, *shape, generator=torch.Generator().manual_seed(NOISE_SEED + call))


def case_config(spec, subsample=10):
    """runner_config plus the fields NCSNRunner.sample() reads, then the case's settings."""
    config = runner_config(spec["name"], spec["batch"], 0, subsample)
    s = config.sampling
    s.fid, s.inpainting, s.interpolation, s.data_init, s.final_only = False, False, False, False, True
    config.fast_fid = argparse.Namespace(pr_nn_k=3)
    for sect in ("data", "model", "sampling"):
        for k, v in spec.get(sect, {}).items():
            setattr(getattr(config, sect), k, v)
    s.num_frames_pred = config.data.num_frames
    return config


def write_checkpoint(folder, config, ckpt, sd_seed, ema_seed):
    """The reference's checkpoint list (:425-433) from two synth seeds -> the file name."""
    model = {"module." + k: v for k, v in synth.make_state_dict(config, seed=sd_seed).items()}
    shadow = synth.make_state_dict(config, seed=ema_seed) if ema_seed is not None else {}
    name = "checkpoint.pt" if ckpt == "latest" else f"checkpoint_{ckpt}.pt"
    torch.save([model, {}, 0, 0, shadow], os.path.join(folder, name))
    return name


def gen_case(case, subsample=10):
    spec = CASES[case]
    R = import_real_runner()
    import models as ref_models
    config = case_config(spec, subsample)
    d, s = config.data, config.sampling
    B = spec["batch"]
    C, nf, nc, S, future = d.channels, d.num_frames, d.num_frames_cond, d.image_size, getattr(d, "num_frames_future", 0)
    T = nc + nf + future
    clips = torch.rand(B, T, C, S, S, generator=torch.Generator().manual_seed(53))      # one batch: a second next() starts the loader over
    ds = torch.utils.data.TensorDataset(clips, torch.zeros(B))
    tmp = tempfile.mkdtemp(prefix="mcvd_sample_")
    log_path, image_folder = os.path.join(tmp, "log"), os.path.join(tmp, "img")
    os.makedirs(log_path), os.makedirs(image_folder)
    args = argparse.Namespace(log_path=log_path, data_path=tmp, image_folder=image_folder, feats_dir=tmp)
    ckpt = "latest" if s.ckpt_id is None else s.ckpt_id
    ema_seed = EMA_SEED if config.model.ema else None
    ckpt_file = write_checkpoint(log_path, config, ckpt, SD_SEED, ema_seed)
    runner = R.NCSNRunner(args, config, None)

    per_call = subsample - 1
    shape = (B, C * nf, S, S)
    st = dict(call=-1, draw=0, noise=None)
    served, zs, calls, sums, grids, grid_nrows, files, fid_rec = [], [], [], [], [], [], [], {}
    printed = io.StringIO()
    real_dt, real_randn, real_save = R.data_transform, torch.randn, torch.save
    real_sampler = ref_models.ddpm_sampler

    def data_transform(cfg, X):
        served.append(X.clone())
        return real_dt(cfg, X)

    def randn(*a, **kw):
        z = real_randn(*a, **kw)
        if "generator" not in kw and z.dim() == 4 and tuple(z.shape) == shape:            # the init z (:1117, :1230)
            zs.append(z.clone())
        return z

    def randn_like(like, *a, **kw):
        z = st["noise"][st["draw"]].to(like)
        st["draw"] += 1
        assert z.shape == like.shape
        return z

    def spy_sampler(x_mod, scorenet, **kw):
        rec = dict(x_init=x_mod.clone(), cond=None if kw.get("cond") is None else kw["cond"].clone(), has_cond_mask="cond_mask" in kw,
                   cond_mask=None if kw.get("cond_mask") is None else kw["cond_mask"].clone(),
                   kwargs={k: v for k, v in kw.items() if k not in ("cond", "cond_mask", "config")})
        st["call"], st["draw"] = st["call"] + 1, 0
        st["noise"] = step_noise(st["call"], per_call, tuple(x_mod.shape))
        sums.append(float(st["noise"].double().sum()))
        calls.append(rec)
        mark = len(printed.getvalue())
        out = real_sampler(x_mod, scorenet, **kw)
        assert st["draw"] == per_call, st["draw"]
        rec["out"] = (out[-1:] if s.fid else out).clone()          # (the FID branch omits final_only and reads the last image alone, :1275)
        rec["log_lines"] = [ln for ln in printed.getvalue()[mark:].splitlines() if ln.startswith("DDPM: ")]
        return out

    def make_grid(tensor, nrow=8, **kw):
        grids.append(tensor.clone())
        grid_nrows.append(int(nrow))
        return torch.zeros(3, 8, 8)

    def save(obj, path, *a, **kw):
        files.append(os.path.basename(path))
        return real_save(obj, path, *a, **kw)

    def get_fid_PR(feats_path, gen_samples, device, k=3):
        fid_rec.update(gen_samples=gen_samples.clone(), k=k)
        return FID_TRIPLE

    torch.manual_seed(1234)                                                               # the DataLoader's shuffles and the init z
    raised = None
    with contextlib.redirect_stdout(printed), mock.patch.object(R, "get_dataset", lambda *a, **kw: (ds, ds)), \
            mock.patch.object(R, "data_transform", data_transform), \
            mock.patch.object(R, "ddpm_sampler", spy_sampler), \
            mock.patch.object(R, "make_grid", make_grid), \
            mock.patch.object(R, "save_image", lambda *a, **kw: None), \
            mock.patch.object(R, "get_feats_path", lambda *a, **kw: "feats"), \
            mock.patch.object(R, "get_fid_PR", get_fid_PR), \
            mock.patch.object(torch, "save", save), \
            mock.patch.object(torch, "randn", randn), \
            mock.patch.object(torch, "randn_like", randn_like):
        try:
            ret = runner.sample()
            assert ret is None
        except NameError as e:                                                            # :1285, FID branch only
            raised = str(e)
    assert (raised is not None) == bool(s.fid) and (raised is None or "precisions" in raised), raised
    n_rounds = (s.num_samples4fid // B) if s.fid else 1
    assert len(calls) == len(zs) == n_rounds, (len(calls), len(zs))
    assert sorted(files) == sorted(os.listdir(image_folder))
    saved = {f: torch.load(os.path.join(image_folder, f), weights_only=True) for f in files}

    has_cond = calls[0]["cond"] is not None
    out = dict(case=case, config_name=spec["name"], overrides={k: dict(spec.get(k, {})) for k in ("data", "model", "sampling")}, batch=B,
               subsample=subsample, sd_seed=SD_SEED, ema_seed=ema_seed, ckpt=ckpt, ckpt_file=ckpt_file, fid=bool(s.fid), n_rounds=n_rounds,
               served=torch.stack(served) if served else None, z=torch.stack(zs), x_init=torch.stack([c["x_init"] for c in calls]),
               call_cond=torch.stack([c["cond"] for c in calls]) if has_cond else None, call_cond_mask=[c["cond_mask"] for c in calls],
               call_has_cond_mask=[c["has_cond_mask"] for c in calls], call_kwargs=[c["kwargs"] for c in calls],
               call_log_lines=[c["log_lines"] for c in calls], call_out=torch.stack([c["out"] for c in calls]),
               noise_seed=NOISE_SEED, noise_sums=sums, grids=grids, grid_nrows=grid_nrows, files=files, saved=saved,
               gen_samples=fid_rec.get("gen_samples"), fid_triple=FID_TRIPLE if s.fid else None, pr_nn_k=fid_rec.get("k"),
               stood_in=sorted(ABSENT))
    tag = f"sample_mode_{case}"
    _save(tag, out)
    sys.stdout.write(f"wrote {tag}.pt: ckpt {ckpt!r} ({ckpt_file}), {len(calls)} sampler calls, {len(served)} batches served, out "
                     f"{tuple(out['call_out'].shape) if torch.is_tensor(out['call_out']) else out['call_out']}, {len(grids)} grids "
                     f"(nrow {sorted(set(grid_nrows))}), files {files}, raised {raised!r}\n")


if __name__ == "__main__":
    torch.set_num_threads(4)
    os.makedirs(OUT, exist_ok=True)
    for c in sys.argv[1:] or list(CASES):
        gen_case(c)
