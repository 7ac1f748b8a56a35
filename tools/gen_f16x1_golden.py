"""The drift of the one-piece fp16 arithmetic ("f16x1"), emulated on the CPU: tests/golden/f16x1_drift.pt.

    PYTHONDONTWRITEBYTECODE=1 python -m tools.gen_f16x1_golden          (CPU only; a few minutes)

BASELINE config 2 (smmnist_big5_ngf96), B = 2, through the CPU oracle (oracle/unet_ref.py, oracle/sampler_ref.py) with the synthetic
weights, inputs and injected noise of tests/golden/smmnist_big5_ngf96_b2.pt, every 3x3 conv with Cin >= 32 -- the GroupNorm-ed ones, the
convs the option may move -- replaced by tests/f16x1_ref.py's restatement of conv_wino2h.cpp's one-piece form (operands rounded where the kernel rounds
them, products accumulated in fp64).  Stored:
    config_name, batch, convs_per_forward
    result                         the emulated final frames of DDPM-100 + denoise                       [B, C, H, W] fp32
    sampler_max_abs / _mean_abs    their deviation from the reference's frames (sampler_ddpm_100.result of the fixture above)
    fwd_max_abs / _mean_abs        one forward's eps (at the fixture's fwd_t) against the reference's fwd_eps
tests/test_gpu_f16x1.py holds the kernel's own deviations to 3 x these.  They are recorded results, not a tolerance anyone chose.
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
STEPS = 100


def main():
    g = torch.load(os.path.join(GOLDEN, "smmnist_big5_ngf96_b2.pt"), weights_only=False)
    config = synth.make_config(g["config_name"])
    sd = synth.make_state_dict(config, seed=123)
    B = g["batch"]
    x, cond = synth.make_inputs(config, B, seed=0)
    noise = synth.make_noise(config, B, STEPS + 1, seed=2)
    orig, count = unet_ref.conv2d, [0]

    def patched(xx, w, b):
        if w.shape[-1] == 3 and w.shape[1] >= 32:
            count[0] += 1
            return f16x1_ref.conv_f16x1(xx, w, b)
        return orig(xx, w, b)
    unet_ref.conv2d = patched
    try:
        with torch.no_grad():
            eps = unet_ref.unet_forward(sd, config, x, g["fwd_t"], cond)
            per_forward = count[0]
            net = unet_ref.OracleScoreNet(config, sd)
            k = [0]

            def fn(i, like):
                k[0] += 1
                return noise[k[0] - 1].to(like)
            t0 = time.time()
            out = sampler_ref.sample(x.clone(), net, cond=cond, kind="ddpm", final_only=True, denoise=True, subsample_steps=STEPS,
                                     clip_before=True, noise_fn=fn)
            print(f"{per_forward} convs per forward emulated, sampler {time.time() - t0:.0f} s")
    finally:
        unet_ref.conv2d = orig
    ref = g["sampler_ddpm_100"]["result"]
    ds, df = (out - ref).abs(), (eps - g["fwd_eps"]).abs()
    fx = dict(config_name=g["config_name"], batch=B, convs_per_forward=per_forward, result=out.float().contiguous(),
              sampler_max_abs=float(ds.max()), sampler_mean_abs=float(ds.mean()), fwd_max_abs=float(df.max()), fwd_mean_abs=float(df.mean()))
    print({k_: v for k_, v in fx.items() if k_ != "result"}, "max|frame|", float(ref.abs().max()), "max|eps|", float(g["fwd_eps"].abs().max()))
    torch.save(fx, os.path.join(GOLDEN, "f16x1_drift.pt"))


if __name__ == "__main__":
    main()
