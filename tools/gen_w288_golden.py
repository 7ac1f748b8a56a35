"""One forward of the REAL reference at the ngf-288 widths of the UCF-101 models: tests/golden/w288_forward.pt.

    PYTHONDONTWRITEBYTECODE=1 python -m tools.gen_w288_golden          (CPU only, needs the reference checkout; about a minute)

The nets are tests/w288_cases.py's: `tiny` / `tiny_spade` at image_size 8, ngf 288, heads of 288 channels, ch_mult [4], one ResBlock per
level, attention at 8 (SPADE: spade_dim 64), and the plain net again with model.cond_emb.  UNetMore_DDPM is imported unmodified
(oracle/gen_golden.py: build_ref_net) and loaded with synth.make_state_dict(config, seed); the weights are never stored.  Per case the file
holds
    seed, batch, x, t, cond (, mask: the cond_mask of the cond_emb case)
    eps                       the reference's output                                                   [B, C * nf, 8, 8]
    tap_temb                  output of all_modules[1], the second Linear of the time embedding         [B, 1152]
    up_block                  index in all_modules of the first ResBlock of the up path (2304 -> 1152)
    tap_up, tap_up_scale      its output flat[::TAP_STRIDE] and max |output| (the whole tensor is 0.6 MB a case)
and, for the plain case, `sampler_ddpm5`: ddpm_sampler(subsample_steps=5, denoise=True, clip_before=True) with the injected noise
synth.make_noise(config, B, 6, seed=2), and the number of draws it took.
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import torch  # noqa: E402

from oracle import synth  # noqa: E402
from oracle.gen_golden import NoiseInjector, build_ref_net, check_names  # noqa: E402
from tests import w288_cases as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def gen_case(case):
    config = W.make_config(case)
    net = build_ref_net(config)
    check_names(net, config)
    missing = net.load_state_dict(synth.make_state_dict(config, seed=W.SEED), strict=False)
    assert not missing.unexpected_keys and set(missing.missing_keys) <= {"betas", "alphas", "alphas_prev", "unet.sigmas"}
    x, cond = synth.make_inputs(config, W.BATCH, seed=0)
    t = torch.tensor([990, 130]).long()
    up = W.first_up_block(config)
    taps, hooks = {}, []
    for i in (1, up):
        hooks.append(net.unet.all_modules[i].register_forward_hook(lambda mod, inp, o, i=i: taps.__setitem__(i, o.detach().clone())))
    kw = {}
    out = dict(seed=W.SEED, batch=W.BATCH, x=x, t=t, cond=cond, up_block=up)
    if case == "condemb":
        out["mask"] = torch.tensor([1, 0], dtype=torch.int32)
        kw["cond_mask"] = out["mask"]
    with torch.no_grad():
        eps = net(x, t, cond=cond, **kw)
    for h in hooks:
        h.remove()
    assert list(taps[1].shape) == [W.BATCH, 1152] and list(taps[up].shape) == [W.BATCH, 1152, 8, 8]
    out.update(eps=eps.clone(), tap_temb=taps[1], tap_up=taps[up].reshape(-1)[::W.TAP_STRIDE].clone(),
               tap_up_scale=float(taps[up].abs().max()))
    if case == "plain":
        import models as ref_models
        inj = NoiseInjector(synth.make_noise(config, W.BATCH, 6, seed=2))
        orig = torch.randn_like
        torch.randn_like = inj
        try:
            res = ref_models.ddpm_sampler(x.clone(), net, cond=cond, final_only=True, denoise=True, subsample_steps=5, clip_before=True,
                                          verbose=False, log=False)
        finally:
            torch.randn_like = orig
        out["sampler_ddpm5"], out["sampler_n_noise"] = res.clone(), inj.k
    print(f"{case}: eps std {float(eps.std()):.4f} max {float(eps.abs().max()):.4f}, up block {up} max {out['tap_up_scale']:.4f}")
    return out


def main():
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    fx = {case: gen_case(case) for case in W.CASES}
    path = os.path.join(GOLDEN, W.FIXTURE)
    torch.save(fx, path)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
