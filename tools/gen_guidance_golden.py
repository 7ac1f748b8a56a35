"""Golden vectors of classifier-free guidance -- build container only (needs the reference checkout).

    PYTHONDONTWRITEBYTECODE=1 python -m tools.gen_guidance_golden

Drives the REAL `ddpm_sampler`, `ddim_sampler` and `FPNDM_sampler` (models/__init__.py) on the CPU with the injected noise sequence
of oracle/gen_golden.py.  The callable they get wraps the real `UNetMore_DDPM` (synthetic weights of oracle/synth.py), exposes the
attributes the three samplers read (`alphas`, `alphas_prev`, `betas`, `type`) and returns

    e_c + (s - 1) * (e_c - e_u),   e_c = net(x, t, cond=cond),   e_u = net(x, t, cond=cond_weak[, cond_mask=mask])

(`cond_mask` only where the net has `cond_emb`).  All cases at B = 2, subsample 10, on the 32 x 32 `oracle.synth` configs.

Fixture tests/golden/guidance.pt (tensors above 64 KB live in companion files, see tests/golden_io.py):
    batch, subsample,
    x_init.<config>, cond.<config>, noise.<config>     the inputs every case of a config shares (synth.make_inputs seed 0, make_noise seed 2)
    cond_weak.<config>.<drop>                          the weak conditioning of every case of that config and drop
    result.<config> [cases of the config, 1, B, C*nf, S, S] fp32, result64.<config> the same runs on the oracle restatement in float64
    cases: [dict(id, config_name, kind ddpm | ddim | fpndm, scale, drop, mask, t_min, denoise, n_noise, row (of result.<config>),
                 ref_dev = max |result - result64|)]
    unguided: {kind: result}  the same samplers on `tiny` handed the bare net (the scale-1 cases must equal these bit for bit)
The reference's network hard-codes float32 in its timestep embedding and cannot run in double: the float64 run is the restatement of
oracle/ (pinned to the reference by tests/test_oracle_golden.py), as for every other `ref32_vs_ref64` number of the fixtures.
"""
import math
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import torch  # noqa: E402

from oracle import sampler_ref, synth, unet_ref  # noqa: E402
from oracle.gen_golden import OUT, REF, NoiseInjector, build_ref_net  # noqa: E402

BATCH, SUBSAMPLE = 2, 10
SPLIT_BYTES = 64 << 10
PART_BYTES = 900 << 10

# (config, drop, sampler kind, scale, sampler kwargs)
CASES = [("tiny", "all", kind, s, {}) for kind in ("ddpm", "ddim", "fpndm") for s in (0.0, 1.0, 2.5)] + [
    ("tiny_condemb", "all", "ddpm", 2.5, {}),
    ("tiny_spade", "past", "ddpm", 2.5, {}),
    ("tiny_spade", "future", "ddpm", 2.5, {}),
    ("tiny", "all", "ddpm", 2.5, dict(t_min=0.3)),
]


def weak_conditioning(config, cond, drop):
    """(cond_weak, mask) in the layout of conditioning_fn (runners/ncsn_runner.py:104-147): [past block | future block]; the mask is
    the keep mask of the past block.  Written out here so the fixture does not depend on the package under test."""
    d = config.data
    n_past, n_future = d.channels * d.num_frames_cond, d.channels * getattr(d, "num_frames_future", 0)
    weak = cond.clone()
    if drop == "all":
        return torch.zeros_like(cond), 0
    if drop == "past":
        weak[:, :n_past] = 0
        return weak, 0
    assert drop == "future" and n_future > 0
    weak[:, n_past:] = 0
    return weak, 1


class Guided:
    """The reference samplers' `scorenet`: the guided combination of two evaluations of `net`."""

    def __init__(self, net, scale, cond_weak, mask, cond_emb):
        self.net, self.scale, self.cond_weak, self.mask, self.cond_emb = net, scale, cond_weak, mask, cond_emb
        self.alphas, self.alphas_prev, self.betas = net.alphas, net.alphas_prev, net.betas
        self.type = getattr(net, "type", None)

    def __call__(self, x, t, cond=None):
        s, weak = self.scale, self.cond_weak.to(x.dtype)
        e_c = self.net(x, t, cond=cond)
        if self.cond_emb:
            e_u = self.net(x, t, cond=weak, cond_mask=torch.full((x.shape[0],), self.mask, dtype=torch.int32))
        else:
            e_u = self.net(x, t, cond=weak)
        return e_c + (s - 1) * (e_c - e_u)


def run_reference(ref_models, kind, scorenet, x, cond, noise, kw):
    inj = NoiseInjector(noise)
    orig = torch.randn_like
    torch.randn_like = inj
    try:
        with torch.no_grad():
            if kind == "fpndm":
                res = ref_models.FPNDM_sampler(x.clone(), scorenet, cond=cond, final_only=True, subsample_steps=SUBSAMPLE, clip_before=True,
                                               verbose=False, log=False)
            else:
                sampler = dict(ddpm=ref_models.ddpm_sampler, ddim=ref_models.ddim_sampler)[kind]
                res = sampler(x.clone(), scorenet, cond=cond, final_only=True, denoise=True, subsample_steps=SUBSAMPLE, clip_before=True,
                              verbose=False, log=False, **kw)
    finally:
        torch.randn_like = orig
    return res.clone(), inj.k


def run_fp64(config, sd, kind, scale, weak, mask, x, cond, noise, kw):
    net64 = unet_ref.OracleScoreNet(config, sd, dtype=torch.float64)
    g64 = Guided(net64, scale, weak.double(), mask, bool(config.model.cond_emb))
    if kind == "fpndm":
        return sampler_ref.fpndm_sample(x.double().clone(), g64, cond=cond.double(), final_only=True, subsample_steps=SUBSAMPLE,
                                        clip_before=True)
    k = [0]

    def fn(i, like):
        k[0] += 1
        return noise[k[0] - 1].to(like.dtype)
    return sampler_ref.sample(x.double().clone(), g64, cond=cond.double(), kind=kind, final_only=True, denoise=True,
                              subsample_steps=SUBSAMPLE, clip_before=True, noise_fn=fn, **kw)


def main():
    sys.path.insert(0, REF)
    import models as ref_models
    out = dict(batch=BATCH, subsample=SUBSAMPLE, cases=[], unguided={})
    nets, results = {}, {}
    for name in sorted({c[0] for c in CASES}):
        config = synth.make_config(name)
        net = build_ref_net(config)
        sd = synth.make_state_dict(config, seed=123)
        net.load_state_dict(sd, strict=False)
        x, cond = synth.make_inputs(config, BATCH, seed=0)
        noise = synth.make_noise(config, BATCH, SUBSAMPLE + 1, seed=2)
        nets[name] = (config, net, sd, x, cond, noise)
        out[f"x_init.{name}"], out[f"cond.{name}"], out[f"noise.{name}"] = x, cond, noise
    config, net, sd, x, cond, noise = nets["tiny"]
    for kind in ("ddpm", "ddim", "fpndm"):
        out["unguided"][kind], _ = run_reference(ref_models, kind, net, x, cond, noise, {})
    for name, drop, kind, scale, kw in CASES:
        config, net, sd, x, cond, noise = nets[name]
        weak, mask = weak_conditioning(config, cond, drop)
        res, n_noise = run_reference(ref_models, kind, Guided(net, scale, weak, mask, bool(config.model.cond_emb)), x, cond, noise, kw)
        res64 = run_fp64(config, sd, kind, scale, weak, mask, x, cond, noise, kw)
        ref_dev = float((res.double() - res64).abs().max())
        cid = f"{name}-{drop}-{kind}-s{scale:g}" + "".join(f"-{k}{v:g}" for k, v in kw.items())
        out[f"cond_weak.{name}.{drop}"] = weak
        results.setdefault(name, []).append((res, res64))
        out["cases"].append(dict(id=cid, config_name=name, kind=kind, scale=scale, drop=drop, mask=mask, t_min=kw.get("t_min", -1),
                                 denoise=kind != "fpndm", n_noise=n_noise, row=len(results[name]) - 1, ref_dev=ref_dev))
        sys.stdout.write(f"  {cid}: range [{res.min():.4f}, {res.max():.4f}], draws {n_noise}, fp32 vs fp64 {ref_dev:.3e}\n")
    for name, rr in results.items():
        out[f"result.{name}"] = torch.stack([r for r, _ in rr])
        out[f"result64.{name}"] = torch.stack([r for _, r in rr])
    os.makedirs(OUT, exist_ok=True)
    for k in [k for k in out if torch.is_tensor(out[k])]:
        v = out[k]
        if v.numel() * v.element_size() > SPLIT_BYTES:
            per = max(1, PART_BYTES // (v[0].numel() * v.element_size()))
            names = []
            for i in range(math.ceil(len(v) / per)):
                names.append(f"guidance.{k}.{i}.pt")
                torch.save(v[i * per:(i + 1) * per].clone(), os.path.join(OUT, names[-1]))
            out[k] = {"parts": names, "dim": 0}
    path = os.path.join(OUT, "guidance.pt")
    torch.save(out, path)
    assert os.path.getsize(path) < 1 << 20, os.path.getsize(path)
    sys.stdout.write(f"wrote guidance.pt ({os.path.getsize(path)} bytes), {len(out['cases'])} cases\n")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
