"""What a guided sampler call costs against the unguided call of twice its batch, one process on one MI355X: profiles/guidance_time.txt.

    python tools/guidance_time.py [--calls 5] [--subsample 100] [--scale 2.5] [--label new] [--out profiles/guidance_time.txt]

Workload: BASELINE config 2 (smmnist_big5_ngf96), DDPM-<subsample> + denoise, the bench's weights and inputs, seeded device noise.
Three legs, each AUTOTUNED in this run by its warm-up call: unguided B = 64, unguided B = 32, guided B = 32 (weak conditioning: zeros).
A guided call at B runs the forwards of an unguided call at 2B; per step it adds a second epsilon read and two more x writes to the
update kernel, so the comparison is guided(32) against unguided(64): the ratio of the medians of `calls` timed calls, each between
device synchronisations.  Needs a GPU; nothing here falls back.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from mcvd_pytorch_amd import HipScoreNet, _lib, ddpm_sampler, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--subsample", type=int, default=100)
    ap.add_argument("--scale", type=float, default=2.5)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance_time.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/guidance_time.py measures on the GPU"
    name = "smmnist_big5_ngf96"
    config = bench.make_config(name)
    config.sampling.subsample = args.subsample
    config.device = "cuda:0"
    net = HipScoreNet(config)
    net.load_state_dict(synthetic.random_state_dict(net, seed=123), strict=True)
    x, cond = (t.cuda() for t in synthetic.random_inputs(config, 0, 64))

    def call(B, seed, **kw):
        return ddpm_sampler(x[:B], net, cond=cond[:B], final_only=True, denoise=True, subsample_steps=args.subsample, clip_before=True,
                            verbose=False, log=False, seed=seed, **kw)[0]

    legs = [("unguided B = 64", 64, {}), ("unguided B = 32", 32, {}), ("guided   B = 32", 32, dict(guidance_scale=args.scale))]
    lines = [f"\n# tools/guidance_time.py [{args.label}]: {name}, DDPM-{args.subsample} + denoise, {torch.cuda.get_device_name(0)}, library "
             f"{os.path.basename(_lib.LIB_PATH)}; every leg autotuned by its warm-up call; median of {args.calls} timed calls"]
    med = {}
    for leg, B, kw in legs:
        call(B, 999, **kw)                                       # warm-up: the autotune of this leg's forward batch
        ts = []
        for i in range(args.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(B, 1000 + i, **kw)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        med[leg] = statistics.median(ts)
        lines.append(f"{leg}: median {1e3 * med[leg]:9.2f} ms   [{', '.join(f'{1e3 * t:.2f}' for t in ts)}]   "
                     f"spread {100 * (max(ts) - min(ts)) / med[leg]:.2f} %")
    r = med["guided   B = 32"] / med["unguided B = 64"]
    lines.append(f"guided(32) / unguided(64) = {r:.4f}   (expected <= 1.03: the forwards are the same, the update kernel reads one more "
                 f"epsilon and writes x three times);  guided(32) / unguided(32) = {med['guided   B = 32'] / med['unguided B = 32']:.4f}")
    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "a").write(txt)


if __name__ == "__main__":
    main()
