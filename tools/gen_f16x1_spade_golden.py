"""The drift of the one-piece fp16 arithmetic ("f16x1") on a SPADE net, emulated on the CPU: tests/golden/f16x1_spade_drift.pt.

    PYTHONDONTWRITEBYTECODE=1 python -m tools.gen_f16x1_spade_golden          (CPU only; some minutes)

BASELINE config 4 (bair_big_spade), B = 2, through the CPU oracle (oracle/unet_ref.py, oracle/sampler_ref.py) with the synthetic weights,
inputs and injected noise of tests/golden/bair_big_spade_b2_fwd.pt / _ddpm100.pt.  The convs the option may move -- the 3x3 convs with a
SPADE norm directly in front: Conv_0 of a ResBlock that does not resample (behind a FIR the conv reads a raw tensor and stays exact),
Conv_1 of every ResBlock, the last conv -- are replaced by tests/f16x1_ref.py's restatement of conv_wino2h.cpp's one-piece form (operands rounded where
the kernel rounds them, products accumulated in fp64).  They are selected by the KEY of their weight, not by its shape: MySPADE's
mlp_gamma / mlp_beta are 3x3 convs over spade_dim = 128 channels too, read a ReLU-ed tensor no norm bounds, and stay exact -- as do
mlp_shared, the stem and the shortcuts.  Stored:
    config_name, batch, steps, convs_per_forward, keys (the weights emulated)
    result                         the emulated final frames of DDPM-<steps> + denoise                    [1, B, C, H, W] fp32
    sampler_max_abs / _mean_abs    their deviation from the reference's frames (`result` of bair_big_spade_b2_ddpm100.pt)
    fwd_reference                  "oracle": the reference's forward fixture holds a strided probe of eps only, so the forward's deviation
                                   is taken against the CPU oracle's eps (which tests/test_oracle_golden.py holds to that probe)
    fwd_max_abs / _mean_abs        one forward's eps (at the fixture's fwd_t) against that
    fwd_probe_max_abs              ... and, at the probe's indices, against the reference's own values
tests/test_gpu_f16_spade.py holds the kernel's own deviations to 3 x these.  They are recorded results, not a tolerance anyone chose.
"""
import os
import sys
import time

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import torch  # noqa: E402

from oracle import sampler_ref, synth, unet_ref  # noqa: E402
from tests import f16x1_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def movable_keys(config):
    """The weight keys of the 3x3 convs with a SPADE norm directly in front (oracle/unet_ref.py: res_block, unet_forward)."""
    mods = unet_ref.module_plan(unet_ref.hot_cfg(config))
    keys = []
    for i, m in enumerate(mods):
        if m["kind"] != "res":
            continue
        if not (m["up"] or m["down"]):
            keys.append(f"unet.all_modules.{i}.Conv_0.weight")
        keys.append(f"unet.all_modules.{i}.Conv_1.weight")
    assert mods[-1]["kind"] == "conv3" and mods[-2]["kind"] == "norm"
    keys.append(f"unet.all_modules.{len(mods) - 1}.weight")
    return keys


def main():
    gf = torch.load(os.path.join(GOLDEN, "bair_big_spade_b2_fwd.pt"), weights_only=False)
    gs = torch.load(os.path.join(GOLDEN, "bair_big_spade_b2_ddpm100.pt"), weights_only=False)
    assert gf["config_name"] == gs["config_name"] and gf["batch"] == gs["batch"] and gs["kind"] == "ddpm"
    config = synth.make_config(gf["config_name"])
    assert unet_ref.hot_cfg(config).spade
    B, steps = gf["batch"], gs["subsample"]
    net = unet_ref.OracleScoreNet(config, synth.make_state_dict(config, seed=123))
    keys = movable_keys(config)
    emulated = {id(net.sd[k]) for k in keys}                      # by identity of the weight the oracle passes: by key
    assert len(emulated) == len(keys)
    x, cond = synth.make_inputs(config, B, seed=0)
    noise = synth.make_noise(config, B, steps + 1, seed=2)
    orig, count = unet_ref.conv2d, [0]

    def patched(xx, w, b):
        if id(w) in emulated:
            assert w.shape[-1] == 3
            count[0] += 1
            return f16x1_ref.conv_f16x1(xx, w, b)
        return orig(xx, w, b)
    with torch.no_grad():
        exact = unet_ref.unet_forward(net.sd, config, x, gf["fwd_t"], cond)
    unet_ref.conv2d = patched
    try:
        with torch.no_grad():
            eps = unet_ref.unet_forward(net.sd, config, x, gf["fwd_t"], cond)
            per_forward = count[0]
            assert per_forward == len(keys), (per_forward, len(keys))
            k = [0]

            def fn(i, like):
                k[0] += 1
                return noise[k[0] - 1].to(like)
            t0 = time.time()
            out = sampler_ref.sample(x.clone(), net, cond=cond, kind="ddpm", final_only=True, denoise=True, subsample_steps=steps,
                                     clip_before=True, noise_fn=fn)
            print(f"{per_forward} convs per forward emulated, sampler {time.time() - t0:.0f} s")
    finally:
        unet_ref.conv2d = orig
    assert k[0] == gs["n_noise"] and out.shape == gs["result"].shape
    p = gf["fwd_eps_probe"]
    ds, df = (out - gs["result"]).abs(), (eps - exact).abs()
    dp = (eps.reshape(-1).double()[p["idx"]].float() - p["sample"]).abs()
    fx = dict(config_name=gf["config_name"], batch=B, steps=steps, convs_per_forward=per_forward, keys=keys, result=out.float().contiguous(),
              sampler_max_abs=float(ds.max()), sampler_mean_abs=float(ds.mean()), fwd_reference="oracle", fwd_max_abs=float(df.max()),
              fwd_mean_abs=float(df.mean()), fwd_probe_max_abs=float(dp.max()))
    print({k_: v for k_, v in fx.items() if k_ not in ("result", "keys")}, "max|frame|", float(gs["result"].abs().max()), "max|eps|",
          float(exact.abs().max()))
    torch.save(fx, os.path.join(GOLDEN, "f16x1_spade_drift.pt"))


if __name__ == "__main__":
    main()
