"""Caller-side glue of the sampling path, restated so the reference's sampling scripts have everything they use around
the sampler: conditioning layout, data transforms and the autoregressive block driver of `NCSNRunner.video_gen`.
Everything stays on the GPU between blocks (the reference moves each block to the CPU and back,
runners/ncsn_runner.py:1521-1539).
"""
from math import ceil

import torch

from .samplers import get_sampler


def _frames_to_channels(frames):
    """[B, T, C, H, W] -> [B, T*C, H, W]: frame-major channel stacking (channel index t*C + c), the layout every tensor of the
    sampling path uses."""
    return frames.flatten(1, 2)


def _keep_mask(n, p_drop, device):
    """Per-sample Bernoulli keep mask (True with probability 1 - p_drop), one torch.rand draw per call as the reference's masks."""
    return torch.rand(n, device=device) > p_drop


def conditioning_fn(config, X, num_frames_pred=0, prob_mask_cond=0.0, prob_mask_future=0.0, conditional=True):
    """Clip [B, T, C, H, W] -> (pred, cond, cond_mask) in the channel layout of the network: pred = the `num_frames_pred` frames after
    the past, cond = [past frames | future frames] with whole samples zeroed by the conditioning masks.  Behaviour of
    NCSNRunner's conditioning_fn (runners/ncsn_runner.py:104-147), including its draw order (cond mask, then future mask), so a
    seeded reference script sees the same masks; `conditional=False` returns the flattened clip alone."""
    d = config.data
    if not conditional:
        return _frames_to_channels(X), None, None
    n_past, n_train, n_future = d.num_frames_cond, d.num_frames, getattr(d, "num_frames_future", 0)
    B, dev = X.shape[0], X.device
    pred = _frames_to_channels(X[:, n_past:n_past + num_frames_pred])
    blocks = [_frames_to_channels(X[:, :n_past])]
    cond_mask = None
    if prob_mask_cond > 0.0:
        keep = _keep_mask(B, prob_mask_cond, dev)
        blocks[0] = blocks[0] * keep.view(B, 1, 1, 1)
        cond_mask = keep.to(torch.int32)
    if n_future > 0:
        if prob_mask_future == 1.0:                   # the future block is dropped for everybody: zeros, whatever the clip holds
            fut = torch.zeros(B, d.channels * n_future, d.image_size, d.image_size, device=dev)
        else:
            start = n_past + n_train
            fut = _frames_to_channels(X[:, start:start + n_future])
            if prob_mask_future > 0.0:
                if getattr(d, "prob_mask_sync", False):
                    if cond_mask is None:
                        raise AttributeError("prob_mask_sync needs prob_mask_cond > 0 (the reference reuses the cond mask there)")
                    keep_f = cond_mask
                else:
                    keep_f = _keep_mask(B, prob_mask_future, dev)
                fut = fut * keep_f.view(B, 1, 1, 1)
        blocks.append(fut)
    return pred, torch.cat(blocks, dim=1) if len(blocks) > 1 else blocks[0], cond_mask


TASKS = ("pred", "interp", "pred_future_masked", "gen")
# (prob_mask_cond, prob_mask_future) each phase of NCSNRunner.video_gen hands conditioning_fn (:1458-1459, :1625-1626, :1798-1799)
_TASK_MASKS = {"pred": (0.0, 0.0), "interp": (0.0, 0.0), "pred_future_masked": (0.0, 1.0), "gen": (1.0, 1.0)}


def _task_frames(config, task):
    """Frames a task produces (:1450-1456, :1621, :1793); ValueError for a task the config's layout cannot run."""
    d, s = config.data, config.sampling
    future = getattr(d, "num_frames_future", 0)
    if task not in _TASK_MASKS:
        raise ValueError(f"unknown task {task!r}; one of {TASKS}")
    if task == "pred" and future > 0:
        raise ValueError("task 'pred' needs data.num_frames_future == 0 (with future frames the reference interpolates, :1453-1456)")
    if task in ("interp", "pred_future_masked") and future == 0:
        raise ValueError(f"task {task!r} needs data.num_frames_future > 0")
    if task == "interp":
        return int(d.num_frames)
    if task == "gen":
        return int(d.num_frames_cond) + int(s.num_frames_pred)
    return int(s.num_frames_pred)


def video_tasks(config):
    """The phases NCSNRunner.video_gen runs on a batch for this config, in its order, as [(task, num_frames_pred), ...]:

      (1) "pred" (num_frames_future == 0, sampling.num_frames_pred frames) or "interp" (future > 0, data.num_frames frames);
      (2) "pred_future_masked" when future > 0, data.prob_mask_future > 0 and not data.prob_mask_sync (sampling.num_frames_pred);
      (3) "gen" when data.prob_mask_cond > 0 (num_frames_cond + sampling.num_frames_pred frames).

    Branch table :1309-1335, phase gates :1444, :1612, :1783.  The reference runs (3) only under `sampling.fvd` and only when
    num_frames_cond + num_frames_pred >= 10 (an FVD rule); neither gate is applied here.  With prob_mask_sync the reference sizes its
    dataloader by the :1406 branch (the :1408 one cannot be reached), but runs the phases of :1326-1329: (1) and (3)."""
    d, s = config.data, config.sampling
    future = getattr(d, "num_frames_future", 0)
    tasks = [("interp" if future > 0 else "pred")]
    if future > 0 and getattr(d, "prob_mask_future", 0.0) > 0.0 and not getattr(d, "prob_mask_sync", False):
        tasks.append("pred_future_masked")
    if getattr(d, "prob_mask_cond", 0.0) > 0.0:
        tasks.append("gen")
    return [(t, _task_frames(config, t)) for t in tasks]


def task_conditioning(config, X, task):
    """Clip [B, T, C, H, W] (network range) -> (real, cond, cond_mask, num_frames_pred) for one phase of `video_tasks`: conditioning_fn
    with that phase's masks -- "pred" / "interp" (0, 0), "pred_future_masked" (0, 1: the future block zeroed), "gen" (1, 1: cond and
    future zeroed, cond_mask all zeros).  The "gen" call draws its cond mask from torch.rand as the reference does."""
    nfp = _task_frames(config, task)
    p_cond, p_future = _TASK_MASKS[task]
    real, cond, cond_mask = conditioning_fn(config, X, num_frames_pred=nfp, prob_mask_cond=p_cond, prob_mask_future=p_future)
    return real, cond, cond_mask, nfp


GUIDANCE_DROPS = ("past", "future", "all")


def guidance_conditioning(config, cond, drop="all"):
    """The weak conditioning of a guided sampler call, `(cond_weak, mask)`, from cond in the layout of `conditioning_fn` ([past block |
    future block], whose cond_mask is the keep mask of the past block): what a net trained with conditioning dropout saw for the dropped
    part of its batches.  Feed it to the samplers as `guidance_cond=cond_weak, guidance_mask=mask`.

      * "past":   the first C * num_frames_cond channels zeroed (prob_mask_cond), mask 0;
      * "future": the trailing C * num_frames_future channels zeroed (prob_mask_future), mask 1; ValueError without future frames;
      * "all":    zeros, mask 0.
    `cond` is not modified."""
    d = config.data
    n_past, n_future = d.channels * d.num_frames_cond, d.channels * getattr(d, "num_frames_future", 0)
    if drop not in GUIDANCE_DROPS:
        raise ValueError(f"unknown guidance drop {drop!r}; one of {GUIDANCE_DROPS}")
    if drop == "future" and n_future == 0:
        raise ValueError("guidance drop 'future' needs data.num_frames_future > 0")
    if cond.dim() != 4 or cond.shape[1] != n_past + n_future:
        raise ValueError(f"cond has shape {tuple(cond.shape)}; expected [B, {n_past + n_future}, S, S]")
    if drop == "all":
        return torch.zeros_like(cond), 0
    weak = cond.clone()
    if drop == "past":
        weak[:, :n_past] = 0
        return weak, 0
    weak[:, n_past:] = 0
    return weak, 1


def _mean_image(config, like):
    m = getattr(config, "image_mean", None)
    return None if m is None else m.to(like.device)[None, ...]


def data_transform(config, X):
    """[0, 1] frames -> the range the network was trained on: the `config.data` switches of datasets/__init__.py:235-249
    (dequantisation noise, `rescaled` to [-1, 1] or the logit transform, minus the dataset's mean image when one is configured)."""
    d = config.data
    if getattr(d, "uniform_dequantization", False):
        X = X / 256.0 * 255.0 + torch.rand_like(X) / 256.0
    if getattr(d, "gaussian_dequantization", False):
        X = X + 0.01 * torch.randn_like(X)
    if getattr(d, "rescaled", False):
        X = 2.0 * X - 1.0
    elif getattr(d, "logit_transform", False):
        Y = 1e-6 + (1.0 - 2.0 * 1e-6) * X
        X = torch.log(Y) - torch.log1p(-Y)
    mean = _mean_image(config, X)
    return X if mean is None else X - mean


def inverse_data_transform(config, X):
    """The inverse map back to [0, 1], clamped (datasets/__init__.py:252-261)."""
    d = config.data
    mean = _mean_image(config, X)
    if mean is not None:
        X = X + mean
    if getattr(d, "logit_transform", False):
        X = torch.sigmoid(X)
    elif getattr(d, "rescaled", False):
        X = 0.5 * (X + 1.0)
    return X.clamp(0.0, 1.0)


@torch.no_grad()
def video_gen(config, scorenet, cond, num_frames_pred=None, init_noise_fn=None, sampler=None, data_init=None, verbose=False,
              log=False, task=None, cond_mask=None, guidance_scale=None, guidance_drop="all", **sampler_kwargs):
    """Autoregressive block loop of NCSNRunner.video_gen (runners/ncsn_runner.py:1476-1569, prediction path: future == 0), kept on
    the device between blocks (the reference moves every block to the CPU and back, :1521-1539).  Returns [B, C*num_frames_pred, S, S].

      * blocks: ceil(num_frames_pred / num_frames), or num_frames_pred when `sampling.one_frame_at_a_time` (:1501-1504);
      * block input: fresh z for every block (:1476, :1551) unless `sampling.init_prev_t` > 0, where block i > 0 restarts from the
        previous block's output and the sampler re-noises it (:1513, models/__init__.py:269-280);
      * cond update (:1528-1539): `cond is None` (unconditional bootstrap) -> cond = gen; one_frame_at_a_time -> drop the oldest
        cond frame, append the first generated frame; else drop the oldest num_frames cond frames, append the newest
        min(num_frames, num_frames_cond) generated frames;
      * `data_init` (sampling.data_init, :1479-1498, :1553-1565): frames `real_init` already in network range, flattened to
        channels as the reference does; block input = sqrt(alpha_0) * real_init1 + sqrt(1 - alpha_0) * z.  The later-block slices
        follow the reference's expressions literally (they index dim 0 there);
      * result: cat(blocks, dim=1)[:, :C*num_frames_pred] (:1569).

      * `config.model.gamma` (:1470-1474, :1518, :1545-1549): every sampler call gets `gamma=True` and the initial z of every block is the
        centred gamma variate Gamma(k_cum[0], rate 1 / theta_t[0]) - k_cum[0] * theta_t[0].  With `data_init` as well the reference
        divides by an undefined `used_alphas` (:1494, NameError): that combination is refused here too.

    `init_noise_fn(block_index, shape, device)` supplies z (default: torch.randn on the device, or the centred gamma variate for a
    `model.gamma` config).  A `seed=` kwarg (on-device Philox step noise) is advanced by one per block, so blocks never share a
    noise stream.

    `task` (one of `video_tasks(config)`, with cond / cond_mask from `task_conditioning`) runs that phase's block loop instead;
    `num_frames_pred` then defaults to the task's frame count.  `task=None` is the loop above, unchanged.
      * "pred": the loop above (future == 0).
      * "interp" (:1444-1569 with future > 0): one block; num_frames_pred > num_frames is refused (ValueError).  Under
        one_frame_at_a_time the reference runs num_frames one-frame blocks with the prediction shift (:1502, :1530-1531), which moves
        the future frame into the past window -- reproduced as it is.
      * "pred_future_masked" (:1612-1720) and "gen" (:1783-1916) with future > 0: the shift keeps the trailing C*future channels (the
        zero future block) at the end of cond (:1700-1708, :1874-1882); "gen" with future == 0 shifts as prediction (:1867-1871).
        Under one_frame_at_a_time that shift grows cond by C*future channels per block and the reference's second sampler call fails
        on the shape: a RuntimeError before the second block here.
    `cond_mask` goes to the sampler as given for block 0 and as ones for every later block (:1885-1886).  It is not routed into the
    forward: the reference samplers take it into **kwargs and drop it (models/__init__.py:207-209), so a `model.cond_emb` net samples
    as if the mask were ones, here as there.  data_init, init_prev_t, model.gamma and the per-block seed mean the same in every task.

    `guidance_scale` (no reference counterpart; None = off, the loop above untouched): every sampler call is guided (samplers.py), its
    weak conditioning rebuilt from the shifted cond of each block, `guidance_conditioning(config, cond, guidance_drop)`.  It needs cond
    (ValueError for the unconditional bootstrap)."""
    d, s = config.data, config.sampling
    C, nf, nc, S = d.channels, d.num_frames, d.num_frames_cond, d.image_size
    future = getattr(d, "num_frames_future", 0)
    if task is None:
        nfp = int(num_frames_pred if num_frames_pred is not None else s.num_frames_pred)
    else:
        task_frames = _task_frames(config, task)                                      # also refuses a task the layout cannot run
        nfp = int(num_frames_pred if num_frames_pred is not None else task_frames)
        if task == "interp" and nfp > nf:                                             # :1456: one block of num_frames frames
            raise ValueError(f"task 'interp' produces at most data.num_frames = {nf} frames, asked for {nfp}")
    keep_future = task in ("pred_future_masked", "gen") and future > 0                # :1700-1708, :1874-1882
    one_at_a_time = bool(getattr(s, "one_frame_at_a_time", False))
    sampler = sampler or get_sampler(config)
    dev = scorenet.device
    if guidance_scale is not None and cond is None:
        raise ValueError("video_gen: guidance_scale needs conditioning frames (cond is None)")
    if cond is not None:
        cond = cond.to(dev).float().contiguous()
        B = cond.shape[0]
    else:
        B = int(sampler_kwargs.pop("batch_size", getattr(s, "batch_size", 1)))
    shape = (B, C * nf, S, S)
    gamma = bool(getattr(config.model, "gamma", False))
    if gamma and data_init is not None:
        raise NameError("name 'used_alphas' is not defined (runners/ncsn_runner.py:1494: the reference cannot run model.gamma with "
                        "sampling.data_init; refused here as well)")
    if init_noise_fn is None:
        if gamma:
            k0, th0 = float(scorenet.k_cum[0]), float(scorenet.theta_t[0])

            def init_noise_fn(i, shp, dv):
                # drawn on the CPU and then moved, as the reference does (:1470-1474, :1545-1549: `Gamma(full(...), full(...)).sample().to(device)`):
                # under torch.manual_seed a reference script and this loop consume the same CPU generator stream
                g = torch.distributions.gamma.Gamma(torch.full(shp, k0), torch.full(shp, 1.0 / th0)).sample().to(dv)
                return g - k0 * th0
        else:
            def init_noise_fn(i, shp, dv):
                return torch.randn(shp, device=dv)
    t_min = getattr(s, "init_prev_t", -1)
    n_iter = nfp if one_at_a_time else ceil(nfp / nf)                                  # :1501-1504
    seed = sampler_kwargs.pop("seed", None)
    sampler_kwargs.pop("gamma", None)                 # decided by config.model.gamma (:1518); a duplicate keyword would be a TypeError below
    real_init = None
    if data_init is not None:
        real_init = data_init.to(dev).float().reshape(len(data_init), -1, S, S)        # conditioning_fn(..., conditional=False) :109-110
        alpha0 = scorenet.alphas[0]

    def init_for(i, real_init1):
        z = init_noise_fn(i, shape, dev)
        if real_init is None:
            return z
        return alpha0.sqrt() * real_init1 + (1 - alpha0).sqrt() * z                   # :1495-1496, :1563-1564

    init = init_for(0, real_init[:, :C * nf] if real_init is not None else None)       # :1488
    cond_width = None if cond is None else cond.shape[1]
    preds, gen = [], None
    for i in range(n_iter):
        x0 = init if (i == 0 or t_min <= 0) else gen                                    # :1513
        kw = dict(sampler_kwargs)
        if seed is not None:
            kw["seed"] = int(seed) + i
        if task is not None and cond is not None and cond.shape[1] != cond_width:       # one_frame_at_a_time + kept future block
            raise RuntimeError(f"task {task!r}, block {i}: the cond shift left {cond.shape[1]} cond channels, the network takes "
                               f"{cond_width} (the reference's sampler call fails here too, :1700-1703, :1874-1877)")
        if guidance_scale is not None:
            weak, weak_mask = guidance_conditioning(config, cond, guidance_drop)
            kw.update(guidance_scale=guidance_scale, guidance_cond=weak, guidance_mask=weak_mask)
        mask = cond_mask if (i == 0 or cond_mask is None) else torch.ones_like(cond_mask)   # :1885-1886
        out = sampler(x0, scorenet, cond=cond, cond_mask=mask, final_only=True, denoise=getattr(s, "denoise", True),
                      subsample_steps=getattr(s, "subsample", None), clip_before=getattr(s, "clip_before", True),
                      t_min=t_min, gamma=gamma, verbose=verbose, log=log, **kw)
        gen = out[-1].reshape(B, C * nf, S, S)                                          # :1521-1522
        preds.append(gen)
        if i == n_iter - 1:
            continue
        if cond is None:                                                                # :1528-1529
            cond = gen
        elif keep_future:                                                               # :1700-1708, :1874-1882
            head = cond[:, C:] if one_at_a_time else cond[:, C * nf:cond.shape[1] - C * future]
            new = gen[:, :C] if one_at_a_time else gen[:, C * max(0, nf - nc):]
            cond = torch.cat([head, new, cond[:, cond.shape[1] - C * future:]], dim=1).contiguous()
        elif one_at_a_time:                                                             # :1530-1531
            cond = torch.cat([cond[:, C:], gen[:, :C]], dim=1).contiguous()
        else:                                                                           # :1532-1535
            cond = torch.cat([cond[:, C * nf:], gen[:, C * max(0, nf - nc):]], dim=1).contiguous()
        real_init1 = None
        if real_init is not None:                                                       # :1553-1557 (dim-0 slices, sic)
            real_init1 = real_init[C * (i + 1):C * (i + 1 + nf)] if one_at_a_time else \
                real_init[(i + 1) * C * nf:(i + 2) * C * nf]
        init = init_for(i + 1, real_init1)
    return torch.cat(preds, dim=1)[:, :C * nfp]                                         # :1569


# seed layout of evaluate_video_gen: (batch, phase) -> seed + ((3 * batch + phase - 1) << _SEED_SHIFT); video_gen adds the block index below it
_SEED_SHIFT = 20
# draw word of the block init noise (kernels/philox.h, "Draw words in use"): bit 41, which no other stream sets
INIT_NOISE_DRAW = 1 << 41


def _format_p(dd):
    """The reference's format_p (:2284).  It formats ckpt as `{v:7d}`, which raises for the "latest" of :1367; a ckpt that is not an int
    is printed as it is."""
    parts = []
    for k, v in dd.items():
        if k == "ckpt":
            parts.append(f"{k}:{v:7d}" if isinstance(v, int) else f"{k}:{v}")
        elif k == "preds_per_test":
            parts.append(f"{k}:{v:3d}")
        elif k == "time":
            parts.append(f"{k}:{v}")
        else:
            parts.append(f"{k}:{v:.4f}")
    return ", ".join(parts)


def _video_gen_branch(config):
    """(name of phase (1), phase (2) aliased, phase (3) aliased) of the six branches that :2169-2190 and :2296-2365 switch on; None for a
    mask combination none of them matches (prob_mask_cond > 0 with future frames and prob_mask_future == 0)."""
    d = config.data
    condp, futrf = float(getattr(d, "prob_mask_cond", 0.0)), int(getattr(d, "num_frames_future", 0))
    futrp, sync = float(getattr(d, "prob_mask_future", 0.0)), bool(getattr(d, "prob_mask_sync", False))
    if condp == 0.0 and futrf == 0:                                  # (1) Prediction
        return "pred", False, False
    if condp == 0.0 and futrf > 0 and futrp == 0.0:                  # (1) Interpolation
        return "interp", False, False
    if condp == 0.0 and futrf > 0 and futrp > 0.0:                   # (1) Interp + (2) Pred
        return "interp", True, False
    if condp > 0.0 and futrf == 0:                                   # (1) Pred + (3) Gen
        return "pred", False, True
    if condp > 0.0 and futrf > 0 and futrp > 0.0 and not sync:       # (1) Interp + (2) Pred + (3) Gen
        return "interp", True, True
    if condp > 0.0 and futrf > 0 and futrp > 0.0 and sync:           # (1) Interp + (3) Gen
        return "interp", False, True
    return None


def video_gen_aliases(config, vid_metrics):
    """The pred_ / interp_ / gen_ keys of vid_metrics.yml (:2296-2365), added to `vid_metrics` in the reference's order: phase (1)'s keys
    under the name of its task, phase (2)'s mse2... as pred_..., phase (3)'s fvd3... as gen_fvd....  A key that is absent (no LPIPS net, an
    FVD gate off, phase (2) not run) is skipped where the reference would raise KeyError."""
    branch = _video_gen_branch(config)
    if branch is None:
        return vid_metrics
    first, second, third = branch

    def alias(prefix, suffix):
        for tail in ("", "_std", "_conf95"):
            for m in ("mse", "psnr", "ssim", "lpips"):
                if f"{m}{suffix}{tail}" in vid_metrics:
                    vid_metrics[f"{prefix}_{m}{tail}"] = vid_metrics[f"{m}{suffix}{tail}"]
        alias_fvd(prefix, suffix)

    def alias_fvd(prefix, suffix):
        for tail in ("", "_traj_mean", "_traj_std", "_traj_conf95"):
            if f"fvd{suffix}{tail}" in vid_metrics:
                vid_metrics[f"{prefix}_fvd{tail}"] = vid_metrics[f"fvd{suffix}{tail}"]
    alias(first, "")
    if second:
        alias("pred", "2")
    if third:
        alias_fvd("gen", "3")
    return vid_metrics


def write_to_yaml(yaml_file, my_dict):
    """NCSNRunner.write_to_yaml (:2867-2877): merged into the file's dict when it exists and written with sorted keys."""
    import os
    import yaml
    if os.path.exists(yaml_file):
        with open(yaml_file, "r") as f:
            old_dict = yaml.load(f, Loader=yaml.FullLoader)
        for key in my_dict.keys():
            old_dict[key] = my_dict[key]
        my_dict = {}
        for key in sorted(old_dict.keys()):
            my_dict[key] = old_dict[key]
    with open(yaml_file, "w") as f:
        yaml.dump(my_dict, f, default_flow_style=False)


def _saved_dicts(config, pred, real, cond_original, pred2, real2, pred_uncond):
    """The dicts the reference saves for one batch (:1985-1993, :2106-2112, :2131-2135, :2157-2159, branches :2169-2190) as
    {file stem: {key: CPU tensor}}: videos_pred {cond, pred, real}, videos_interp {cond, pred, real, futr}, videos_gen {gen}.  `real` is
    padded with zero frames when it is shorter than `pred` (:1988-1990); with future frames `cond` is split into cond and futr (:1992-1993),
    and phase (2)'s dict keeps phase (1)'s cond frames, as the reference's closure does."""
    C, nc, future = config.data.channels, config.data.num_frames_cond, getattr(config.data, "num_frames_future", 0)
    cpu = lambda t: t.detach().to("cpu")                 # noqa: E731
    cond, futr = cond_original, None
    if real.shape[1] < pred.shape[1]:
        real = torch.cat([real, torch.zeros(real.shape[0], pred.shape[1] - real.shape[1], real.shape[2], real.shape[3], device=real.device)], dim=1)
    if future > 0:
        cond, futr = torch.tensor_split(cond, (nc * C,), dim=1)
    branch = _video_gen_branch(config)
    out = {}
    if branch is None:
        return out
    first, second, third = branch
    if first == "pred":
        out["videos_pred"] = {"cond": cpu(cond), "pred": cpu(pred), "real": cpu(real)}
    else:
        out["videos_interp"] = {"cond": cpu(cond), "pred": cpu(pred), "real": cpu(real), "futr": cpu(futr)}
    if second and pred2 is not None:
        out["videos_pred"] = {"cond": cpu(cond), "pred": cpu(pred2), "real": cpu(real2)}
    if third and pred_uncond is not None:
        out["videos_gen"] = {"gen": cpu(pred_uncond)}
    return out


def _finish_video_gen(config, metrics, ckpt, train, out_dir, start_time, log, write):
    """The part of NCSNRunner.video_gen after its loop (:2192-2368) on a complete `metrics`: summary, embeddings file, log lines, aliases, YAML."""
    import datetime
    import os
    import time
    import numpy as np
    from .metrics import fvd_gates
    summary = metrics.summary()
    if summary is None:                                               # :2192
        return None
    vid_metrics = {"ckpt": ckpt, **summary}
    if not train and write and out_dir is not None and any(fvd_gates(config)):         # :2271-2278
        np.savez(os.path.join(out_dir, f"video_embeddings_{ckpt}.npz"), **metrics.embeddings())
    elapsed = str(datetime.timedelta(seconds=(time.time() - start_time)))[:-3]          # :2283
    log(f"elapsed: {elapsed}, {_format_p(vid_metrics)}")                               # :2285
    if train:                                                         # :2288-2289
        return vid_metrics
    vid_metrics["time"] = elapsed                                     # :2294
    video_gen_aliases(config, vid_metrics)                            # :2296-2365
    log(f"elapsed: {elapsed}, {_format_p(vid_metrics)}")                               # :2367
    if write and out_dir is not None:                                 # :2368
        write_to_yaml(os.path.join(out_dir, "vid_metrics.yml"), vid_metrics)
    return vid_metrics


@torch.no_grad()
def evaluate_video_gen(config, scorenet, batches, *, ckpt="latest", train=False, max_data_iter=None, preds_per_test=None,
                       lpips=None, fvd=None, fvd_batch=10, data_init_batches=None, out_dir=None, sampler=None,
                       init_noise_fn=None, seed=None, shard=None, metrics=None, log=None, guidance_scale=None, guidance_drop="all"):
    """NCSNRunner.video_gen (runners/ncsn_runner.py:1304-2368), the mode `main.py --video_gen` runs, as one call: every batch of `batches`
    through the phases of `video_tasks(config)`, the frames of each phase into a `VideoMetrics`, and the reference's vid_metrics dict back.
    Frames stay on the device from the sampler to the metrics (the reference's per-block `.to('cpu')`, :1523, is not reproduced).

      * returns {} when neither sampling.ssim nor sampling.fvd is set (:1340-1343); asserts data.num_frames_cond > 0 (:1356);
      * train=True (the call of the training loop, :497): one batch and preds_per_test = 1 (:1345-1348); else sampling.max_data_iter and
        sampling.preds_per_test (:1351-1352) unless `max_data_iter=` / `preds_per_test=` say otherwise;
      * batches: any iterable of clip batches `x` or `(x, _)`, x [b, T, C, S, S] in [0, 1] as a dataset yields them before data_transform:
        the caller's loader, with batch_size = sampling.batch_size // preds_per_test as :1413 sizes it.  Each batch is moved to the device
        once, repeat_interleave(preds_per_test, dim=0) (:1392-1395) and data_transform (:1442); the loop stops at max_data_iter (:1437-1440);
      * phase (1) (:1444-1609): task_conditioning "pred" (num_frames_future == 0) or "interp", video_gen(task=...), inverse_data_transform,
        metrics.update(pred01, real01, phase=1, cond01=cond_original);
        phase (2) under future > 0 and prob_mask_future > 0 and not prob_mask_sync (:1615-1616): "pred_future_masked",
        metrics.update(..., phase=2, cond01=cond_original2);
        phase (3) only under calc_fvd3 of metrics.fvd_gates (:1787): "gen" with num_frames_cond + sampling.num_frames_pred frames (:1793),
        metrics.update_gen(pred_uncond01);
      * the sampler calls get verbose = log = not train, as :1516 and :1519 pass them;
      * sampling.data_init (:1479-1489, :1646-1656, :1818-1828): every phase that runs takes the next batch of `data_init_batches` (an
        iterable of `x` or `(x, _)`, sampling.batch_size clips as :1418 sizes it) and starts it over when it runs out, so it must be
        re-iterable.  With model.gamma the reference fails on an undefined name (:1496); refused as in video_gen;
      * metrics: a ready VideoMetrics or a stand-in with update, update_gen, summary and embeddings (and state / merged under
        torch.distributed).  Default: VideoMetrics(config, preds_per_test, scorenet, lpips=lpips, fvd=fvd, fvd_batch=fvd_batch).
        sampling.fvd without `fvd=` (and without `metrics=`) is a ValueError: the package loads no detector;
      * after the loop (:2192-2368): None where phase (1) could not calculate (:2192), else {'ckpt': ckpt, **metrics.summary()}; unless
        `train` also 'time' and the pred_ / interp_ / gen_ aliases of :2296-2365 (`video_gen_aliases`; absent keys are skipped).  `log`
        (default logging.info) receives the reference's "elapsed: ..., {format_p}" lines (:2285, :2367);
      * out_dir: videos_pred_{ckpt}.pt / videos_interp_{ckpt}.pt / videos_gen_{ckpt}.pt (:2106-2112, :2131-2135, :2157-2159) for the batches
        `i == 0 or preds_per_test == 1` (:1984), each overwriting the last as in the reference; video_embeddings_{ckpt}.npz under :2271 and
        vid_metrics.yml through `write_to_yaml`.  GIFs, PNGs, captions and plots are not written.

    Noise.  Without `seed=` the block init z is video_gen's default (torch.randn on the device, the centred gamma variate under model.gamma)
    and the step noise the samplers' own.  With `seed=` both are Philox streams keyed by the GLOBAL row: (batch i, phase p) samples under
    seed + ((3 i + p - 1) << 20), video_gen adds the block index, the step noise is the samplers' `seed` / `sample_offset` stream and the
    block init z is mcvd_randn's layout at the draw word INIT_NOISE_DRAW (2^41, registered in kernels/philox.h).  `init_noise_fn(block,
    shape, device)` replaces the init z in either case; `sampler=` replaces get_sampler(config).

    Sharding.  shard=(rank, world), or with shard=None the rank and world of an initialised torch.distributed.  A rank takes the CLIPS
    dist.shard_rows(n_clips, rank, world) of every batch, so a clip's preds_per_test rows stay together; global row = begin * preds_per_test
    + local row goes to the samplers as sample_offset.  A shard needs `seed=` (ValueError: torch's generator is not row-keyed), and with
    model.gamma an `init_noise_fn`.  Under torch.distributed the ranks exchange metrics.state() (and the tensors of the saved dicts) with ONE
    all_gather_object after the loop, VideoMetrics.merged reassembles the global order, every rank returns the same dict -- the single-rank
    one, bit for bit -- and rank 0 writes the files.  A shard without a process group returns {'shard': (rank, world), 'state':
    metrics.state(), 'saved': {file stem: tensors}} for the caller to merge (VideoMetrics.merged(config, states).summary()).
    data_transform's dequantisation noise is torch's and not row-keyed: a sharded run of such a config is not the single-rank one.

    Guidance.  `guidance_scale` / `guidance_drop` go to video_gen in phases (1) and (2).  Phase (3) stays unguided: its cond is all zeros
    already, guidance would double its cost and change nothing."""
    import logging
    import os
    import time
    import torch.distributed as tdist
    from . import metrics as M
    from .dist import shard_rows
    log = log or logging.info
    d, s = config.data, config.sampling
    calc_ssim = getattr(s, "ssim", False)
    calc_fvd = getattr(s, "fvd", False)
    if not calc_fvd and calc_ssim is False:                           # :1340-1343
        return {}
    calc_fvd3 = M.fvd_gates(config)[2]                                # :1311-1337
    if train:                                                         # :1345-1348
        assert scorenet is not None and ckpt is not None
        max_data_iter, preds_per_test = 1, 1
    else:                                                             # :1350-1352
        max_data_iter = s.max_data_iter if max_data_iter is None else max_data_iter
        preds_per_test = getattr(s, "preds_per_test", 1) if preds_per_test is None else preds_per_test
    start_time = time.time()
    ppt = int(preds_per_test)
    conditional = d.num_frames_cond > 0                               # :1355-1356
    assert conditional, f"Video generating model has to be conditional! num_frames_cond has to be > 0! Given {d.num_frames_cond}"
    future = getattr(d, "num_frames_future", 0)
    prob_mask_future = getattr(d, "prob_mask_future", 0.0)
    second_calc = future > 0 and prob_mask_future > 0.0 and not getattr(d, "prob_mask_sync", False)      # :1615-1616
    gamma = bool(getattr(config.model, "gamma", False))
    use_data_init = bool(getattr(s, "data_init", False))
    if use_data_init:
        if gamma:
            raise NameError("name 'used_alphas' is not defined (runners/ncsn_runner.py:1496: the reference cannot run model.gamma with "
                            "sampling.data_init; refused here as well)")
        if data_init_batches is None:
            raise ValueError("evaluate_video_gen: sampling.data_init is set: data_init_batches is needed")
    if calc_fvd and fvd is None and metrics is None:
        raise ValueError("evaluate_video_gen: sampling.fvd is set: a detector is needed (fvd=); the package loads none")

    in_group = tdist.is_available() and tdist.is_initialized()
    if shard is None:
        shard = (tdist.get_rank(), tdist.get_world_size()) if in_group else (0, 1)
    rank, world = int(shard[0]), int(shard[1])
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"evaluate_video_gen: shard = {shard!r} is not (rank, world) with 0 <= rank < world")
    exchange = world > 1 and in_group and (rank, world) == (tdist.get_rank(), tdist.get_world_size())
    if world > 1 and seed is None:
        raise ValueError("evaluate_video_gen: a sharded evaluation needs seed= (the Philox streams are keyed by the global row; torch's "
                         "generator is not)")
    if world > 1 and gamma and init_noise_fn is None:
        raise ValueError("evaluate_video_gen: a sharded evaluation of a model.gamma config needs init_noise_fn (the default gamma init "
                         "is drawn from torch's CPU generator, which is not row-keyed)")

    net = scorenet.module if hasattr(scorenet, "module") else scorenet                 # :1389
    dev = net.device
    if metrics is None:
        metrics = M.VideoMetrics(config, preds_per_test=ppt, scorenet=None if getattr(net, "plan_only", False) else net,
                                 lpips=lpips, fvd=fvd, fvd_batch=fvd_batch)
    C, S = d.channels, d.image_size
    init_iter = [None]

    def next_data_init():                                             # :1480-1486: a loader that has run out is started over
        for attempt in range(2):
            if init_iter[0] is None:
                init_iter[0] = iter(data_init_batches)
            try:
                b = next(init_iter[0])
                return b[0] if isinstance(b, (list, tuple)) else b
            except StopIteration:
                init_iter[0] = None
        raise ValueError("evaluate_video_gen: data_init_batches is empty")

    def run_phase(i, phase, task, cond, cond_mask, begin, rows, nfp):
        """One phase's block loop on this rank's rows -> frames in [0, 1]."""
        data_init = None
        if use_data_init:                                             # :1487-1489
            data_init = data_transform(config, next_data_init().to(dev))[begin * ppt:begin * ppt + rows]
        if rows == 0:                                                 # an empty shard samples nothing
            return torch.zeros((0, C * nfp, S, S), device=dev)
        kw, noise_fn = {}, init_noise_fn
        if seed is not None:
            phase_seed = int(seed) + ((3 * i + phase - 1) << _SEED_SHIFT)
            kw = dict(seed=phase_seed, sample_offset=begin * ppt)
            if noise_fn is None and not gamma:
                noise_fn = lambda blk, shp, dv: _philox_init(net, phase_seed + blk, begin * ppt, shp, dv)      # noqa: E731
        if guidance_scale is not None and phase != 3:
            kw.update(guidance_scale=guidance_scale, guidance_drop=guidance_drop)
        pred = video_gen(config, scorenet, cond, task=task, cond_mask=cond_mask, data_init=data_init, sampler=sampler,
                         init_noise_fn=noise_fn, verbose=not train, log=not train, **kw)
        return inverse_data_transform(config, pred)

    saved = {}
    for i, batch in enumerate(batches):
        if i >= max_data_iter:                                        # :1439-1440
            break
        x = (batch[0] if isinstance(batch, (list, tuple)) else batch).to(dev)
        begin, end = shard_rows(len(x), rank, world)
        real_ = x[begin:end].repeat_interleave(ppt, dim=0)            # :1392-1395, this rank's clips
        rows = len(real_)
        real_ = data_transform(config, real_)                         # :1442

        # (1) prediction, or interpolation with future frames (:1444-1609)
        task1 = "pred" if future == 0 else "interp"
        real, cond, cond_mask, nfp = task_conditioning(config, real_, task1)            # :1458-1459
        real = inverse_data_transform(config, real)
        cond_original = inverse_data_transform(config, cond.clone())
        pred = run_phase(i, 1, task1, cond, cond_mask, begin, rows, nfp)
        metrics.update(pred, real, phase=1, cond01=cond_original)

        # (2) prediction with the future block masked (:1612-1778)
        pred2 = real2 = None
        if second_calc:
            real2, cond2, cond_mask2, nfp2 = task_conditioning(config, real_, "pred_future_masked")      # :1625-1626
            real2 = inverse_data_transform(config, real2)
            cond_original2 = inverse_data_transform(config, cond2.clone())
            pred2 = run_phase(i, 2, "pred_future_masked", cond2, cond_mask2, begin, rows, nfp2)
            metrics.update(pred2, real2, phase=2, cond01=cond_original2)

        # (3) unconditional generation, for its FVD alone (:1783-1916, :1974-1982)
        pred_uncond = None
        if calc_fvd3:
            _, cond_fvd, cond_mask_fvd, nfp3 = task_conditioning(config, real_, "gen")  # :1798-1799
            pred_uncond = run_phase(i, 3, "gen", cond_fvd, cond_mask_fvd, begin, rows, nfp3)
            metrics.update_gen(pred_uncond)

        if out_dir is not None and (i == 0 or ppt == 1):              # :1984
            saved.update(_saved_dicts(config, pred, real, cond_original, pred2, real2, pred_uncond))
            if world == 1:
                for stem, dd in saved.items():
                    torch.save(dd, os.path.join(out_dir, f"{stem}_{ckpt}.pt"))

    if world > 1 and not exchange:
        return {"shard": (rank, world), "state": metrics.state(), "saved": saved}
    write = True
    if exchange:
        got = [None] * world
        tdist.all_gather_object(got, (metrics.state(), saved))        # the one collective of a sharded evaluation
        metrics = type(metrics).merged(config, [g[0] for g in got], scorenet=getattr(metrics, "scorenet", None))
        write = rank == 0
        if write and out_dir is not None:
            for stem in got[0][1]:
                dd = {k: torch.cat([g[1][stem][k] for g in got], dim=0) for k in got[0][1][stem]}
                torch.save(dd, os.path.join(out_dir, f"{stem}_{ckpt}.pt"))
    return _finish_video_gen(config, metrics, ckpt, train, out_dir, start_time, log, write)


def _philox_init(net, seed, sample_offset, shape, dev):
    """Standard normals of `shape` = [B, ...] on the device from the library's Philox stream (mcvd_randn): row b is the stream of
    (seed, sample_offset + b, INIT_NOISE_DRAW), whatever the batch it is drawn in."""
    import ctypes as C
    from . import _lib
    z = torch.empty(shape, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        net._bind_stream()
        _lib.check(_lib.lib.mcvd_randn(net._ctx, C.c_void_p(z.data_ptr()), C.c_uint64(seed), C.c_uint64(sample_offset),
                                       C.c_uint64(INIT_NOISE_DRAW), shape[0], z[0].numel()), "randn")
    return z


def _apply_ema_shadow(net, shadow):
    """EMAHelper.register / load_state_dict(shadow) / ema(net) of NCSNRunner.test (:2388-2392, models/ema.py:9-29): every parameter that
    requires grad takes shadow[name] (bare names: the helper unwraps DataParallel); states[0] is not read."""
    for name, p in net.named_parameters():
        if p.requires_grad:
            p.data.copy_(shadow[name].to(device=p.device, dtype=p.dtype))
    net._loaded = True                       # every parameter now holds a checkpoint value (a missing name raised KeyError above)
    net.mark_dirty()


@torch.no_grad()
def test_checkpoints(config, scorenet, batches, log_path, ckpts=None, loss_fn=None, log=None):
    """The loop of NCSNRunner.test() (runners/ncsn_runner.py:2370-2430): for each checkpoint_{ckpt}.pt in `log_path`, the DSM loss of
    every batch and their average -> {ckpt: average test loss}.

      * ckpts: default range(test.begin_ckpt, test.end_ckpt + 1, getattr(test, "freq", 5000));
      * weights: with model.ema the EMA shadow states[-1] (register, load_state_dict, ema), else load_state_dict(states[0]);
      * batches: any iterable of (x, y) with x [B, T, C, H, W] in [0, 1] (the reference's DataLoader), iterated once per checkpoint;
        each x goes through data_transform and conditioning_fn(num_frames_pred=data.num_frames, prob_mask_cond, prob_mask_future,
        conditional = num_frames_cond > 0), then `loss_fn` (default anneal_dsm_score_estimation) with the reference's keywords;
      * the average as the reference forms it: a Python-float sum of the fp32 batch values in batch order, divided by the batch count.
        The batch values stay on the device until the checkpoint is done (one synchronisation per checkpoint);
      * `log` (default logging.info) receives "ckpt: {ckpt}, average test loss: {mean}" per checkpoint, the reference's line."""
    import logging
    import os
    from .losses import anneal_dsm_score_estimation
    loss_fn = loss_fn or anneal_dsm_score_estimation
    log = log or logging.info
    t, d, m = config.test, config.data, config.model
    training = getattr(config, "training", None)
    if ckpts is None:
        ckpts = range(t.begin_ckpt, t.end_ckpt + 1, getattr(t, "freq", 5000))
    net = scorenet.module if hasattr(scorenet, "module") else scorenet
    conditional = d.num_frames_cond > 0
    out = {}
    for ckpt in ckpts:
        states = torch.load(os.path.join(log_path, f"checkpoint_{ckpt}.pt"), map_location="cpu", weights_only=False)
        if getattr(m, "ema", False):
            _apply_ema_shadow(net, states[-1])
        else:
            net.load_state_dict(states[0])
        net.eval()
        values = []
        for x, _ in batches:
            x = data_transform(config, x.to(net.device))
            x, cond, cond_mask = conditioning_fn(config, x, num_frames_pred=d.num_frames, prob_mask_cond=getattr(d, "prob_mask_cond", 0.0),
                                                 prob_mask_future=getattr(d, "prob_mask_future", 0.0), conditional=conditional)
            values.append(loss_fn(scorenet, x, labels=None, cond=cond, cond_mask=cond_mask,
                                  loss_type=getattr(training, "loss_type", "a"), gamma=getattr(m, "gamma", False),
                                  L1=getattr(training, "L1", False), all_frames=getattr(m, "output_all_frames", False)).reshape(()))
        mean_loss = 0.
        for v in (torch.stack(values).cpu().tolist() if values else []):      # test_loss.item() per batch, in batch order
            mean_loss += v
        mean_loss /= len(values)                                                # an empty loader divides by zero, as the reference
        log("ckpt: {}, average test loss: {}".format(ckpt, mean_loss))
        out[ckpt] = mean_loss
    return out


@torch.no_grad()
def fast_fid(config, scorenet, real, detector=None, cond_batches=None, ckpts=None, ckpt_dir=None, out_dir=None, no_pr=False,
             init_noise_fn=None, sampler=None, log=None):
    """The checkpoint sweep of NCSNRunner.fast_fid (runners/ncsn_runner.py:2432-2586): for each checkpoint, `fast_fid.num_samples` frames
    sampled on the device and scored against `real` with FID and the improved precision and recall ->
    {"fids": {ckpt: v}, "precisions": {ckpt: v}, "recalls": {ckpt: v}} (the last two empty with `no_pr`).

      * ckpts: default range(fast_fid.begin_ckpt, fast_fid.end_ckpt + 1, getattr(fast_fid, "freq", 5000)); checkpoint_{ckpt}.pt is read from
        `ckpt_dir` -- with model.ema the EMA shadow states[-1] (register, load_state_dict, ema), else load_state_dict(states[0]) (:2489-2498);
      * sampling (:2502-2551): num_iters = num_samples // batch_size sampler calls of fast_fid.batch_size rows.  z: torch.randn on the device
        (`init_noise_fn(i, shape, device)` replaces it); cond: the next batch of `cond_batches` -- any iterable of (x, y) with x
        [B, T, C, H, W] in [0, 1], started over when it runs out (:2524-2530) -- through data_transform and conditioning_fn, cut to
        batch_size rows; `sampler` (default get_sampler(config)) with final_only=True and sampling.denoise / subsample / clip_before and
        model.gamma; inverse_data_transform; at the end everything reshaped to (-1, C, S, S).  The samples stay on the device;
      * scoring: metrics.fid_pr(real, samples, detector, k=fast_fid.pr_nn_k) -- `real` is the dataset's features (a tensor or a .pt / .pth
        path) or images --, or with `no_pr` metrics.fid_from_stats(real, features of the samples) with `real` = (mu, sigma) or an .npz path.
        The detector is any callable -- the reference's is metrics.FidInception with the caller's weights (see metrics.fid_pr); the
        dataset feature files and the stats download of get_feats_path /
        get_stats_path stay with the caller;
      * files, only with `out_dir`: samples_{ckpt}.pt (CPU tensor) and, without `no_pr`, feats_{ckpt}.pt are written, and reused when present,
        features first, then samples (:2477-2484) -- a checkpoint whose features are there is neither loaded nor sampled.  The image grid,
        the pickles and the YAML files are not written;
      * `log` (default logging.info) receives the reference's "ckpt: ..., fid: ..." line per checkpoint.

    Three defects of the reference are documented and not reproduced: `cond_mask` is unbound for an unconditional config (:2536) -- None is
    passed; the model.gamma branch reads an undefined `real` (:2516) -- z is drawn as video_gen draws it for gamma, the centred variate
    Gamma(k_cum[0], rate 1 / theta_t[0]) - k_cum[0] theta_t[0] on the CPU generator; a cond batch shorter than fast_fid.batch_size
    mis-shapes the sampler call -- ValueError.  With `no_pr` and cached features the reference hands get_fid a .pt path, which it refuses
    (:197); here the cached features are scored.
    `fast_fid.ensemble` and model.version SMLD raise NotImplementedError (the NCSN nets of fast_ensemble_fid are not constructible here)."""
    import logging
    import os
    from . import metrics
    log = log or logging.info
    ff, d, s, m = config.fast_fid, config.data, config.sampling, config.model
    if getattr(ff, "ensemble", False):
        raise NotImplementedError("fast_fid.ensemble (fast_ensemble_fid, :2588) builds NCSN nets, which are not on the HIP path (DESIGN.md section 8)")
    if str(getattr(m, "version", "DDPM")).upper() == "SMLD":
        raise NotImplementedError("fast_fid with model.version SMLD is not on the HIP path (DESIGN.md section 8)")
    batch = int(ff.batch_size)
    if batch < 1:
        raise ValueError(f"fast_fid.batch_size must be at least 1, got {batch}")
    num_iters = int(ff.num_samples) // batch
    if num_iters < 1:
        raise ValueError(f"fast_fid.num_samples = {ff.num_samples} is smaller than fast_fid.batch_size = {batch}: nothing would be sampled")
    if ckpts is None:
        ckpts = range(ff.begin_ckpt, ff.end_ckpt + 1, getattr(ff, "freq", 5000))
    ckpts = list(ckpts)
    conditional = d.num_frames_cond > 0
    if no_pr:
        if not (isinstance(real, str) and real.endswith(".npz")) and not (isinstance(real, (tuple, list)) and len(real) == 2):
            raise ValueError("fast_fid(no_pr=True): `real` must be (mu, sigma) or the path of an .npz with the keys mu and sigma")
    elif isinstance(real, str):
        if not (real.endswith(".pt") or real.endswith(".pth")):
            raise ValueError(f"fast_fid: {real!r} is not a .pt or .pth path of features")
    elif not torch.is_tensor(real) or real.dim() not in (2, 4):
        raise ValueError("fast_fid: `real` must be features [n, dims], images [n, C, H, W] or a .pt / .pth path of features")
    elif real.dim() == 4 and detector is None:
        raise ValueError("fast_fid: `real` holds images: a detector is needed (e.g. FidInception(...).load_state_dict(weights))")

    def cached(kind, ckpt):
        path = None if out_dir is None else os.path.join(out_dir, f"{kind}_{ckpt}.pt")
        return path, path is not None and os.path.exists(path)
    for ckpt in ckpts:                                        # every argument error before any device work
        if cached("feats", ckpt)[1]:
            continue
        if detector is None:
            raise ValueError(f"fast_fid: ckpt {ckpt} has no cached features: a detector is needed to score its samples (e.g. FidInception(...).load_state_dict(weights))")
        if cached("samples", ckpt)[1]:
            continue
        if ckpt_dir is None:
            raise ValueError(f"fast_fid: ckpt {ckpt} has to be sampled: ckpt_dir is needed")
        if conditional and cond_batches is None:
            raise ValueError("fast_fid: data.num_frames_cond > 0: cond_batches is needed")

    net = scorenet.module if hasattr(scorenet, "module") else scorenet
    dev = net.device
    C, nf, S = d.channels, d.num_frames, d.image_size
    shape = (batch, C * nf, S, S)
    gamma = bool(getattr(m, "gamma", False))
    cond_iter = [None]

    def next_cond():
        for attempt in range(2):                              # :2524-2530: a loader that has run out is started over
            if cond_iter[0] is None:
                cond_iter[0] = iter(cond_batches)
            try:
                return next(cond_iter[0])[0]
            except StopIteration:
                cond_iter[0] = None
        raise ValueError("fast_fid: cond_batches is empty")

    def draw_z(i):
        if init_noise_fn is not None:
            return init_noise_fn(i, shape, dev)
        if gamma:                                             # as video_gen (:1470-1474); the reference's own line reads an undefined `real`
            k0, th0 = float(net.k_cum[0]), float(net.theta_t[0])
            g = torch.distributions.gamma.Gamma(torch.full(shape, k0), torch.full(shape, 1.0 / th0)).sample().to(dev)
            return g - k0 * th0
        return torch.randn(shape, device=dev)

    score_net = None if getattr(net, "plan_only", False) else net       # the scores run on the net's context and stream
    out = {"fids": {}, "precisions": {}, "recalls": {}}
    for ckpt in ckpts:
        feats_path, have_feats = cached("feats", ckpt)
        samples_path, have_samples = cached("samples", ckpt)
        save_feats_path = None
        if have_feats:                                        # :2477-2479
            gen = feats_path
        elif have_samples:                                    # :2482-2484
            gen = torch.load(samples_path, map_location="cpu", weights_only=True).to(dev)
            save_feats_path = feats_path
        else:
            states = torch.load(os.path.join(ckpt_dir, f"checkpoint_{ckpt}.pt"), map_location="cpu", weights_only=False)
            if getattr(m, "ema", False):
                _apply_ema_shadow(net, states[-1])
            else:
                net.load_state_dict(states[0])
            net.eval()
            run = sampler or get_sampler(config)
            parts = []
            for i in range(num_iters):
                z = draw_z(i)
                cond = None
                if conditional:
                    x = data_transform(config, next_cond().to(dev))
                    _, cond, _ = conditioning_fn(config, x, conditional=True)
                    if len(cond) < batch:
                        raise ValueError(f"fast_fid: a cond batch of {len(cond)} rows is shorter than fast_fid.batch_size = {batch}")
                    cond = cond[:batch]                       # :2534
                all_samples = run(z, scorenet, cond=cond, cond_mask=None, final_only=True, denoise=getattr(s, "denoise", True),
                                  subsample_steps=getattr(s, "subsample", None), clip_before=getattr(s, "clip_before", True),
                                  verbose=getattr(ff, "verbose", False), gamma=gamma)
                final = all_samples[-1].reshape(all_samples[-1].shape[0], C * nf, S, S)       # :2545-2546
                parts.append(inverse_data_transform(config, final))
            gen = torch.cat(parts, dim=0).reshape(-1, C, S, S)                                 # :2551
            if samples_path is not None:
                torch.save(gen.detach().cpu(), samples_path)
            save_feats_path = feats_path
        if no_pr:                                             # :2562-2567
            feats = metrics.get_activations(gen, detector, 50)
            fid = metrics.fid_from_stats(real, feats, scorenet=score_net)
            out["fids"][ckpt] = fid
            log("ckpt: {}, fid: {}".format(ckpt, fid))
        else:                                                 # :2572-2579
            k = ff.pr_nn_k
            fid, precision, recall = metrics.fid_pr(real, gen, detector, k=k, save_feats_path=save_feats_path,
                                                    scorenet=score_net)
            out["fids"][ckpt], out["precisions"][ckpt], out["recalls"][ckpt] = fid, precision, recall
            log("ckpt: {}, fid: {}, precision: {}, recall: {}".format(ckpt, fid, precision, recall))
    return out


def stretch_image(X, ch, imsize):
    """[B, T*ch, imsize, imsize] -> [B, ch, imsize, T*imsize]: the frames of each row side by side, left to right (stretch_image,
    runners/ncsn_runner.py:150-151).  Reshapes and permutes only, on the device X is on."""
    return X.reshape(len(X), -1, ch, imsize, imsize).permute(0, 2, 1, 4, 3).reshape(len(X), ch, -1, imsize).permute(0, 1, 3, 2)


@torch.no_grad()
def sample(config, scorenet, batches=None, *, cond_batches=None, ckpt_dir=None, real=None, detector=None, out_dir=None, sampler=None,
           init_noise_fn=None, seed=None, shard=None, log=None):
    """NCSNRunner.sample() (runners/ncsn_runner.py:914-1301), the mode `main.py --sample` runs, as one call, up to the tensors the reference
    hands to make_grid and torch.save.  Returns a dict where the reference returns None; frames stay on the device (the `.to('cpu')` of
    :1142 and :1273 is not reproduced).

      * checkpoint (:915-932): ckpt = "latest" when sampling.ckpt_id is None, else the id.  With `ckpt_dir`, checkpoint.pt or
        checkpoint_{ckpt}.pt is loaded through checkpoint.load_states_into: states[0] ('module.' keys), then with model.ema the EMA shadow
        states[-1].  Without `ckpt_dir` the net is used as it is;
      * batches: any iterable of `x` or `(x, _)`, x [B, T, C, S, S] in [0, 1] with B = sampling.batch_size: the caller's loader (the
        reference builds it with shuffle=True; the order is the caller's).  Another batch length is a ValueError (the reference
        mis-shapes its sampler call);
      * plain branch (`not sampling.fid`, :1096-1188): with data_init or a conditional config one batch goes through data_transform and
        conditioning_fn(num_frames_pred=data.num_frames).  z is torch.randn on the device, under model.gamma the centred variate
        Gamma(k_cum[0], rate 1 / theta_t[0]) - k_cum[0] theta_t[0] drawn as video_gen and fast_fid draw it; `init_noise_fn(0, shape,
        device)` replaces z.  Under sampling.data_init the sampler starts from sqrt(alphas[0]) real + sqrt(1 - alphas[0]) z.  The sampler
        call carries the kwargs of :1135-1142 -- cond, cond_mask, n_steps_each, step_lr, verbose=True, final_only, denoise,
        subsample_steps, clip_before, log=True, gamma -- and, without final_only, steps_on_device=True;
      * the result: 'ckpt'; with final_only 'samples' = stretch_image(inverse_data_transform(frames [B, C nf, S, S])), else 'steps', the
        same of every step image in order; 'nrow' (:1156, :1170).  A conditional config adds (:1175-1188) the stretched 'real' and
        'cond' ('futr' too with future frames, split off cond at num_frames_cond C channels), 'padding' = 0.5 ones(B, C, S, 2),
        'full_row' = cat([cond, padding, real, padding, sample(, futr)], -1) -- the tensor the reference hands to make_grid, where
        `sample` is the last step's image -- and 'nrow_full' (:1183);
      * FID branch (`sampling.fid`, :1190-1301): n_rounds = num_samples4fid // batch_size rounds.  Each draws z (`init_noise_fn(round,
        shape, device)`); under data_init takes the next batch of `batches`, started over when it runs out, and mixes it in, its cond
        serving as cond (:1244); otherwise a conditional config takes the next batch of `cond_batches`, started over likewise; calls the
        sampler with verbose=False, log=True; inverse_data_transform.  The rounds are concatenated on the device to 'samples'
        [n_rounds B, C nf, S, S] -- not reshaped to (-1, C, S, S) as fast_fid does -- and scored with metrics.fid_pr(real, samples,
        detector, k=fast_fid.pr_nn_k), `real` and `detector` as in fast_fid -> {'ckpt', 'fids': {ckpt: v}, 'precisions': {ckpt: v},
        'recalls': {ckpt: v}, 'samples'}.  `log` (default logging.info) receives the reference's "ckpt: ..., fid: ..." line;
      * out_dir: what the reference torch.save()s, as CPU tensors -- samples_{ckpt}.pt, or samples_{i:04d}.pt per step, and under a
        conditional config samples_full_{ckpt}.pt (the same `sample`, :1188); in the FID branch samples_{ckpt}.pt.  'files' lists the
        names in the order written.  No PNG, no make_grid, no pickles and no YAML.

    Noise.  Without `seed=` the init z is as above and the step noise the samplers' own.  With `seed=` both are Philox streams keyed by
    the GLOBAL row, as in evaluate_video_gen: the init z is mcvd_randn's layout at the draw word INIT_NOISE_DRAW, the step noise the
    samplers' `seed` / `sample_offset` stream; the plain branch runs under `seed`, FID round i under seed + (i << 20).

    Sharding.  shard=(rank, world): the rank takes the rows dist.shard_rows(B, rank, world) of every batch and of z (`init_noise_fn` is
    then asked for the rank's shape) and hands the first of them to the samplers as sample_offset.  It needs `seed=` and, under
    model.gamma, an `init_noise_fn` (ValueError otherwise).  The rank returns its rows and 'shard': (rank, world); no collective is
    made, nothing is scored and no file is written: the caller concatenates -- in the FID branch round by round, a rank's 'samples'
    holding its rows of round 0, then of round 1, ... ('rounds' says how many).

    Defects of the reference that are documented and not reproduced: `cond_mask` is unbound at :1135 for an unconditional config without
    data_init -- None is passed; model.gamma with data_init reads an undefined `used_alphas` (:1127, :1250) -- refused, as video_gen
    refuses :1496; :1147 reshapes a step image to (B, C, S, S), which raises for data.num_frames > 1 -- reshaped to C nf, as :1162 does;
    the FID branch stops with a NameError at :1285 (`precisions` and `recalls` are never defined) -- here they are filled; its sampler
    call omits final_only, so every step goes to the CPU and only the last is used -- final_only=True is passed.  sampling.inpainting
    and sampling.interpolation call the Langevin samplers with `sigmas`, which is commented out at :934-935: both raise
    NotImplementedError, and so does model.version SMLD."""
    import logging
    import os
    from math import sqrt
    from . import metrics
    from .checkpoint import load_states_into
    from .dist import shard_rows
    log = log or logging.info
    d, s, m = config.data, config.sampling, config.model
    if str(getattr(m, "version", "DDPM")).upper() == "SMLD":
        raise NotImplementedError("sample with model.version SMLD is not on the HIP path (DESIGN.md section 8)")
    fid = bool(getattr(s, "fid", False))
    if not fid and getattr(s, "inpainting", False):
        raise NotImplementedError("sampling.inpainting: the reference calls anneal_Langevin_dynamics_inpainting, a Langevin sampler of the "
                                  "SMLD nets (:979), which is not on the HIP path (DESIGN.md section 8)")
    if not fid and getattr(s, "interpolation", False):
        raise NotImplementedError("sampling.interpolation: the reference calls anneal_Langevin_dynamics_interpolation, a Langevin sampler of "
                                  "the SMLD nets (:1060), which is not on the HIP path (DESIGN.md section 8)")
    gamma = bool(getattr(m, "gamma", False))
    data_init = bool(getattr(s, "data_init", False))
    if gamma and data_init:
        raise NameError("name 'used_alphas' is not defined (runners/ncsn_runner.py:1127, :1250: the reference cannot run model.gamma with "
                        "sampling.data_init; refused here as well)")
    rank, world = (0, 1) if shard is None else (int(shard[0]), int(shard[1]))
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"sample: shard = {shard!r} is not (rank, world) with 0 <= rank < world")
    if world > 1 and seed is None:
        raise ValueError("sample: a sharded run needs seed= (the Philox streams are keyed by the global row; torch's generator is not)")
    if world > 1 and gamma and init_noise_fn is None:
        raise ValueError("sample: a sharded run of a model.gamma config needs init_noise_fn (the default gamma init is drawn from torch's "
                         "CPU generator, which is not row-keyed)")
    conditional = d.num_frames_cond > 0                               # :950
    future = getattr(d, "num_frames_future", 0)                       # :954
    B = int(s.batch_size)
    if B < 1:
        raise ValueError(f"sample: sampling.batch_size must be at least 1, got {B}")
    if fid:
        n_rounds = int(s.num_samples4fid) // B                        # :1191-1192
        if n_rounds < 1:
            raise ValueError(f"sample: sampling.num_samples4fid = {s.num_samples4fid} is smaller than sampling.batch_size = {B}: nothing "
                             "would be sampled")
        if data_init and batches is None:
            raise ValueError("sample: sampling.fid with sampling.data_init: batches is needed")
        if conditional and not data_init and cond_batches is None:
            raise ValueError("sample: sampling.fid with data.num_frames_cond > 0: cond_batches is needed")
        if world == 1 and real is None:
            raise ValueError("sample: sampling.fid: `real` is needed (the data set's features, a .pt / .pth path of them, or images)")
    elif (data_init or conditional) and batches is None:
        raise ValueError("sample: sampling.data_init or data.num_frames_cond > 0: batches is needed")

    ckpt = "latest" if getattr(s, "ckpt_id", None) is None else s.ckpt_id               # :915-921
    net = scorenet.module if hasattr(scorenet, "module") else scorenet                   # :947
    if ckpt_dir is not None:
        name = "checkpoint.pt" if ckpt == "latest" else f"checkpoint_{ckpt}.pt"
        states = torch.load(os.path.join(ckpt_dir, name), map_location="cpu", weights_only=False)
        load_states_into(net, states, use_ema=bool(getattr(m, "ema", False)))          # :926-932
    net.eval()                                                                           # :945
    dev = net.device
    C, nf, nc, S = d.channels, d.num_frames, d.num_frames_cond, d.image_size
    begin, end = shard_rows(B, rank, world)
    rows = end - begin
    shape = (rows, C * nf, S, S)
    run = sampler or get_sampler(config)

    def loader(source, what):
        """next() over `source`, started over when it runs out (:1235-1241, :1256-1262); every batch must hold B clips."""
        it = [None]

        def take():
            for attempt in range(2):
                if it[0] is None:
                    it[0] = iter(source)
                try:
                    b = next(it[0])
                    break
                except StopIteration:
                    it[0] = None
            else:
                raise ValueError(f"sample: {what} is empty")
            x = b[0] if isinstance(b, (list, tuple)) else b
            if len(x) != B:
                raise ValueError(f"sample: a batch of {what} holds {len(x)} clips, sampling.batch_size is {B} (the reference's sampler call "
                                 "would be mis-shaped)")
            return data_transform(config, x.to(dev)[begin:end])
        return take

    def draw_z(i, call_seed):
        if init_noise_fn is not None:
            return init_noise_fn(i, shape, dev)
        if gamma:                                                     # :1112-1115, :1225-1228, drawn as video_gen draws it
            k0, th0 = float(net.k_cum[0]), float(net.theta_t[0])
            g = torch.distributions.gamma.Gamma(torch.full(shape, k0), torch.full(shape, 1.0 / th0)).sample().to(dev)
            return g - k0 * th0
        if call_seed is not None:
            return _philox_init(net, call_seed, begin, shape, dev)
        return torch.randn(shape, device=dev)                         # :1117, :1230

    def mixed(x0, z):                                                 # :1126-1128, :1249-1251
        alpha = net.alphas[0]
        return alpha.sqrt() * x0 + (1 - alpha).sqrt() * z

    def noise_kw(call_seed):
        return {} if call_seed is None else dict(seed=call_seed, sample_offset=begin)

    common = dict(n_steps_each=s.n_steps_each, step_lr=s.step_lr, denoise=s.denoise, subsample_steps=getattr(s, "subsample", None),
                  clip_before=getattr(s, "clip_before", True), log=True, gamma=gamma)
    out = {"ckpt": ckpt}
    if world > 1:
        out["shard"] = (rank, world)
    files = []

    def stretched_01(frames):
        """Network-range frames [n, C T, S, S] -> [0, 1] frames side by side (an empty shard has no rows to infer T from)."""
        if len(frames) == 0:
            return frames.new_zeros((0, C, S, frames.shape[1] // C * S))
        return stretch_image(inverse_data_transform(config, frames), C, S)

    def save(tensor, name):
        if out_dir is not None and world == 1:
            torch.save(tensor.detach().to("cpu"), os.path.join(out_dir, name))
            files.append(name)

    if not fid:                                                       # :1096-1188
        x_real = cond = cond_mask = None
        if data_init or conditional:                                  # :1098-1103
            x_real, cond, cond_mask = conditioning_fn(config, loader(batches, "batches")(), num_frames_pred=nf, conditional=conditional)
        call_seed = None if seed is None else int(seed)
        z = draw_z(0, call_seed)
        init = mixed(x_real, z) if data_init else z                   # :1121-1130
        final_only = bool(s.final_only)
        C_nf = C * nf
        images = []
        if rows > 0:                                                  # (an empty shard samples nothing)
            extra = {} if final_only else dict(steps_on_device=True)
            all_samples = run(init, scorenet, cond=cond, cond_mask=cond_mask, verbose=True, final_only=final_only, **common, **extra,
                              **noise_kw(call_seed))                  # :1135-1142
            images = [all_samples[-1]] if final_only else list(all_samples)
        nrow = ceil(sqrt(nf * B) / nf)                                # :1156, :1170
        stretched = []
        for i, frames in enumerate(images):                           # :1145-1173
            frames = frames.reshape(frames.shape[0], C_nf, S, S)      # :1162 (:1147 names C alone: see the docstring)
            stretched.append(stretched_01(frames))
            save(stretched[-1], f"samples_{ckpt}.pt" if final_only else "samples_{:04d}.pt".format(i))
        if not stretched:
            stretched = [torch.zeros((0, C, S, nf * S), device=dev)]
        last = stretched[-1]
        if final_only:
            out["samples"] = last
        else:
            out["steps"] = stretched
        out["nrow"] = nrow
        if conditional:                                               # :1175-1188
            real01 = stretched_01(x_real)
            if future > 0:
                cond, futr = torch.tensor_split(cond, (nc * C,), dim=1)
                futr = stretched_01(futr)
            cond01 = stretched_01(cond)
            padding = 0.5 * torch.ones(len(real01), C, S, 2, device=dev)
            width = nc + nf * 2 + future
            out["real"], out["cond"] = real01, cond01
            if future > 0:
                out["futr"] = futr
            out["padding"] = padding
            out["full_row"] = torch.cat([cond01, padding, real01, padding, last] + ([futr] if future > 0 else []), dim=-1)
            out["nrow_full"] = ceil(sqrt(width * B) / width)          # :1183
            save(last, f"samples_full_{ckpt}.pt")                     # :1188 saves `sample`, not the full row
        out["files"] = files
        return out

    # ---- FID branch (:1190-1301)
    take_init = loader(batches, "batches") if data_init else None
    take_cond = loader(cond_batches, "cond_batches") if (conditional and not data_init) else None
    parts = []
    for i in range(n_rounds):                                         # :1216
        call_seed = None if seed is None else int(seed) + (i << _SEED_SHIFT)
        z = draw_z(i, call_seed)
        cond = None
        if data_init:                                                 # :1234-1251
            x_real, cond, _ = conditioning_fn(config, take_init(), num_frames_pred=nf, conditional=conditional)
            init = mixed(x_real, z)
        else:
            init = z
            if conditional:                                           # :1255-1265
                _, cond, _ = conditioning_fn(config, take_cond(), num_frames_pred=nf, conditional=conditional)
        if rows == 0:
            parts.append(torch.zeros(shape, device=dev))
            continue
        all_samples = run(init, scorenet, cond=cond, verbose=False, final_only=True, **common, **noise_kw(call_seed))      # :1267-1273
        final = all_samples[-1].reshape(all_samples[-1].shape[0], C * nf, S, S)                                           # :1275-1276
        parts.append(inverse_data_transform(config, final))
    gen_samples = torch.cat(parts, dim=0)                             # :1278
    out["samples"] = gen_samples
    if world > 1:
        out["rounds"] = n_rounds
        out["files"] = files
        return out
    k = config.fast_fid.pr_nn_k                                       # :1283
    score_net = None if getattr(net, "plan_only", False) else net
    fid_v, precision, recall = metrics.fid_pr(real, gen_samples, detector, k=k, scorenet=score_net)      # :1284
    out["fids"], out["precisions"], out["recalls"] = {ckpt: fid_v}, {ckpt: precision}, {ckpt: recall}
    log("ckpt: {}, fid: {}, precision: {}, recall: {}".format(ckpt, fid_v, precision, recall))           # :1286
    save(gen_samples, f"samples_{ckpt}.pt")                           # :1301
    out["files"] = files
    return out


def nearest_neighbors(samples, data_batches, detector, k=10, n_samples=10, out_path=None, scorenet=None):
    """The loop of get_nearest_neighbors (evaluation/nearest_neighbor.py:70-114): the `k` data images nearest, in the detector's feature
    space, to each of the first `n_samples` rows of `samples` (a tensor, or the path of fast_fid's samples_{ckpt}.pt) or to its mirrored
    copy -> metrics.NearestNeighbors.result(): indices, distances, neighbors and plot_data (sample | k neighbours per row of the
    reference's grid).  data_batches: any iterable of `x` or `(x, _)`, as a DataLoader gives, x [B, C, H, W] in [0, 1]; every batch goes
    through the detector and the search once and may then be freed -- the data set is never resident.  out_path: plot_data, indices and
    distances (CPU tensors) as one .pt.  The PNG grid, the data-set table of the script's __main__ and an Inception stay with the caller
    (DESIGN.md section 8)."""
    from . import metrics
    nn = metrics.NearestNeighbors(samples, detector, k=k, n_samples=n_samples, scorenet=scorenet)
    for batch in data_batches:
        nn.update(batch[0] if isinstance(batch, (list, tuple)) else batch)
    out = nn.result()
    if out_path is not None:
        torch.save({key: out[key].detach().cpu() for key in ("plot_data", "indices", "distances")}, out_path)
    return out


def frames_to_uint8(scorenet, frames01, channels):
    """[B, T*C, H, W] frames in [0, 1] (after `inverse_data_transform`) -> uint8 [B, T, H, W, C] on the device: the packing the
    reference applies to every frame before it writes GIFs / PNGs (`(frame * 255).astype('uint8')` on the HWC view,
    runners/ncsn_runner.py:2019-2062).  The grid / caption drawing around it (torchvision make_grid, cv2.putText) is host-side
    presentation and stays with the caller."""
    import ctypes as C
    from . import _lib
    f = frames01.to(device=scorenet.device, dtype=torch.float32).contiguous()
    B, TC, H, W = f.shape
    if TC % channels:
        raise ValueError(f"{TC} channels is not a multiple of {channels}")
    out = torch.empty((B, TC // channels, H, W, channels), dtype=torch.uint8, device=f.device)
    with torch.cuda.device(f.device):
        scorenet._bind_stream()
        _lib.check(_lib.lib.mcvd_pack_frames_u8(scorenet._ctx, C.c_void_p(f.data_ptr()), C.c_void_p(out.data_ptr()), B, TC // channels,
                                                channels, H, W), "pack_frames_u8")
    return out


def save_video_pred(path, cond, pred, real):
    """The on-disk result of NCSNRunner.video_gen: torch.save({"cond", "pred", "real"}) of the [0,1]-range CPU tensors
    (runners/ncsn_runner.py:2106-2112, `videos_pred_<ckpt>.pt`), so downstream metric scripts read our output unchanged."""
    to_cpu = lambda t: None if t is None else t.detach().to("cpu")
    torch.save({"cond": to_cpu(cond), "pred": to_cpu(pred), "real": to_cpu(real)}, path)
    return path
