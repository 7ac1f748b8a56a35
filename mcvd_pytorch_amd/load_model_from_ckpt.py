"""The library surface of the reference's load_model_from_ckpt.py (:39-112) on the HIP path, under the reference's names, so a notebook
or script written against that file runs on this package by changing its import:

    from mcvd_pytorch_amd.load_model_from_ckpt import load_model, get_sampler, init_samples
    scorenet, config = load_model("/path/to/logs/checkpoint.pt", "cuda:0")
    sampler_fn = get_sampler(config)
    frames01 = sampler_fn(init_samples(len(cond), config), scorenet, cond, cond_mask)       # CPU tensor in [0, 1]

`checkpoint.load_model(ckpt_path, config, device)` (config passed explicitly, the net alone returned) keeps its signature; this module
is the variant that reads `config.yml` beside the checkpoint, as the reference file does.
"""
import os
from functools import partial

import torch

from .checkpoint import load_states_into
from .config import dict2namespace
from .runner import inverse_data_transform
from .samplers import ddim_sampler, ddpm_sampler, fpndm_sampler
from .scorenet import HipScoreNet


def load_model(ckpt_path, device="cuda:0"):
    """(scorenet, config) of a checkpoint (:39-61): `config.yml` in the checkpoint's folder -- the plain dict main.py dumps there --
    through dict2namespace, config.device = device, a HipScoreNet with states[0] loaded (strict=False, 'module.' prefixes accepted) and,
    with config.model.ema, the EMA shadow states[-1] over its parameters (EMAHelper.register / load_state_dict / ema), in eval mode.
    The reference wraps the net in DataParallel on a GPU; the HipScoreNet is returned as it is (the samplers accept either)."""
    import yaml
    with open(os.path.join(os.path.dirname(ckpt_path), "config.yml"), "r") as f:
        config = yaml.safe_load(f)
    if not isinstance(config, dict):
        raise ValueError(f"config.yml beside {ckpt_path!r} does not hold a mapping")
    config = dict2namespace(config)
    config.device = torch.device(device) if not isinstance(device, torch.device) else device
    scorenet = HipScoreNet(config, config.device)
    states = torch.load(ckpt_path, map_location="cpu", weights_only=False)
    load_states_into(scorenet, states, use_ema=bool(getattr(config.model, "ema", False)))
    scorenet.eval()
    return scorenet, config


def get_sampler_from_config(config):
    """The sampler of config.model.version (:64-76), bound to the config: DDPM -> ddpm_sampler, DDIM -> ddim_sampler, FPNDM ->
    fpndm_sampler.  The version is compared as written, as the reference does (runner.get_sampler upper-cases it).  SMLD (annealed
    Langevin dynamics) is not on the HIP path: NotImplementedError, as for any other version (the reference
    leaves `sampler` unbound there)."""
    version = getattr(config.model, "version", "DDPM")
    if version == "DDPM":
        return partial(ddpm_sampler, config=config)
    if version == "DDIM":
        return partial(ddim_sampler, config=config)
    if version == "FPNDM":
        return partial(fpndm_sampler, config=config)
    raise NotImplementedError(f"sampler version {version!r} is not on the HIP path (SMLD: out of scope, DESIGN.md section 8)")


def get_sampler(config):
    """sampler_fn(init, scorenet, cond, cond_mask, subsample=sampling.subsample, verbose=False) -> CPU frames in [0, 1] (:79-94): the
    config's sampler with the reference's bound keywords (n_steps_each, step_lr, just_beta=False, final_only=True, sampling.denoise,
    sampling.clip_before, log=False, model.gamma), its last entry moved to the CPU and through inverse_data_transform.  With
    verbose=False the whole step loop runs on the device.  Further keywords (seed=, sample_offset=, noise=) go to the sampler."""
    sampler = get_sampler_from_config(config)
    s = config.sampling
    sampler_partial = partial(sampler, n_steps_each=getattr(s, "n_steps_each", 0), step_lr=getattr(s, "step_lr", 0.0), just_beta=False,
                              final_only=True, denoise=s.denoise, subsample_steps=getattr(s, "subsample", None),
                              clip_before=getattr(s, "clip_before", True), verbose=False, log=False,
                              gamma=getattr(config.model, "gamma", False))

    def sampler_fn(init, scorenet, cond, cond_mask, subsample=getattr(s, "subsample", None), verbose=False, **kwargs):
        init = init.to(config.device)
        cond = cond.to(config.device)
        if cond_mask is not None:
            cond_mask = cond_mask.to(config.device)
        return inverse_data_transform(config, sampler_partial(init, scorenet, cond=cond, cond_mask=cond_mask, subsample_steps=subsample,
                                                              verbose=verbose, **kwargs)[-1].to("cpu"))
    return sampler_fn


def init_samples(n_init_samples, config, net=None):
    """Initial samples [n, C * num_frames, S, S] on the CPU (:97-112), for the branches that can run in the reference: torch.randn for
    DDPM / DDIM / FPNDM.  Its model.gamma branch reads an undefined `net` (:107); with `net=` (the scorenet) it is the centred variate
    Gamma(k_cum[0], rate 1 / theta_t[0]) - k_cum[0] theta_t[0] as video_gen draws it, on the CPU generator.  Its SMLD branch reads an
    undefined `self` (:104) and the SMLD samplers are not on the HIP path: refused."""
    version = getattr(config.model, "version", "DDPM")
    d = config.data
    shape = (n_init_samples, d.channels * d.num_frames, d.image_size, d.image_size)
    if version == "SMLD":
        raise NotImplementedError("init_samples: model.version SMLD is not on the HIP path (DESIGN.md section 8)")
    if version not in ("DDPM", "DDIM", "FPNDM"):
        raise NotImplementedError(f"init_samples: unknown model.version {version!r}")
    if getattr(config.model, "gamma", False):
        if net is None:
            raise NameError("name 'net' is not defined (load_model_from_ckpt.py:107: the reference's gamma branch cannot run; pass net=)")
        net = net.module if hasattr(net, "module") else net
        k0, th0 = float(net.k_cum[0]), float(net.theta_t[0])
        z = torch.distributions.gamma.Gamma(torch.full(shape, k0), torch.full(shape, 1.0 / th0)).sample()
        return z - k0 * th0
    return torch.randn(shape)
