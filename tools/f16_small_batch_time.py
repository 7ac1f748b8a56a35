"""What f16x2 / f16x1 buy on the small per-GPU-batch configs, one process per config on one MI355X: profiles/f16_small_batch_time.txt.

    python tools/f16_small_batch_time.py --config bair_big_spade|cityscapes_big [--rounds 3] [--calls 1] [--subsample 100]
                                         [--label new] [--out profiles/f16_small_batch_time.txt] [--frames FILE] [--save-tables DIR]

Workload: BASELINE config 4 (bair_big_spade, SPADE, B = 16) or 5 (cityscapes_big, B = 8, autoregressive), DDPM-<subsample> + denoise, the
bench's batch, weights and inputs.  Four legs -- default, f16x2, f16x1, both -- each AUTOTUNED in this run (first round; the table is kept
and re-installed in the later rounds) and ALTERNATED over `rounds` rounds of one warm-up call and `calls` timed sampler calls between
device synchronisations.  Reported per leg: frames/s (mean, every round's figure, the spread (max - min) / mean of the rounds) and how
many 3x3 convs ran each kernel id.  Boxes differ by +- 4 %: a leg is compared with the default leg of the same process, and with the
same leg of ANOTHER BUILD of the library only when that build was measured the same way on the same box (MCVD_LIB_PATH names the other
build, --label tells the sections apart; tools/gpu_ab_lib.sh is the bench-level form of the same comparison).

--frames FILE: the frames of one sampler call under the COMMITTED default table (profiles/tune_<config>_B<b>_bf16x3.json: what bench.py
pins), fixed seed, are written to FILE if it does not exist, else compared with it bit by bit -- two builds whose default arithmetic is
the same must agree exactly.  (The autotuned default leg may pick other fp32-equivalent kernels from run to run: no bits to compare.)

Config 4 also records the deviation of the f16x1 frames from the REAL reference's at B = 2 (tests/golden/bair_big_spade_b2_ddpm100.pt,
injected noise), as profiles/f16x1_drift.txt does for config 2.  Needs a GPU; nothing here falls back.
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from mcvd_pytorch_amd import HipScoreNet, _lib, ddpm_sampler, synthetic, video_gen  # noqa: E402

LEGS = [("default", dict(f16x2=0, f16x1=0)), ("f16x2", dict(f16x2=1, f16x1=0)), ("f16x1", dict(f16x2=0, f16x1=1)), ("both", dict(f16x2=1, f16x1=1))]


def conv3_ids(net):
    """kernel id that ran -> number of 3x3 conv ops (the cond-only prep convs included: they ran once, for this cond)"""
    n = _lib.lib.mcvd_model_profile_read(net._model, None, None, None, None, None, 0)
    info, ran = (C.c_int * 8)(), []
    for i in range(n):
        _lib.check(_lib.lib.mcvd_model_op_info(net._model, i, info), "op_info")
        if info[0] == 3 and info[2] == 3:
            ran.append(_lib.lib.mcvd_model_op_kernel(net._model, i))
    return {k: ran.count(k) for k in sorted(set(ran))}


def drift_config4(lines):
    from oracle import synth
    g = torch.load(os.path.join(ROOT, "tests", "golden", "bair_big_spade_b2_ddpm100.pt"), weights_only=False)
    config = synth.make_config(g["config_name"])
    config.device = "cuda:0"
    net = HipScoreNet(config)
    net.load_state_dict(synth.make_state_dict(config, seed=123), strict=True)
    net.eval()
    x, cond = synth.make_inputs(config, g["batch"], seed=0)
    noise = synth.make_noise(config, g["batch"], g["subsample"] + 1, seed=2).cuda()
    lines.append(f"\n## deviation from the REAL reference's frames, config 4 at B = {g['batch']}, DDPM-{g['subsample']} + denoise, injected noise (max|frame| "
                 f"{g['result'].abs().max().item():.3f}); kernels autotuned at B = {g['batch']}")
    lines.append("#                  max-abs      mean-abs     3x3 convs per kernel id")
    for leg, opts in LEGS:
        for k, v in opts.items():
            net.set_option(k, v)
        out = ddpm_sampler(x.cuda(), net, cond=cond.cuda(), denoise=True, subsample_steps=g["subsample"], clip_before=True, verbose=False, log=False,
                           noise=noise, final_only=True)[-1:].cpu()
        d = (out - g["result"]).abs()
        lines.append(f"{leg:12s}  {d.max().item():.3e}    {d.mean().item():.3e}    {conv3_ids(net)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True, choices=["bair_big_spade", "cityscapes_big"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--subsample", type=int, default=100)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--frames", default=None)
    ap.add_argument("--save-tables", default=None, help="directory for tune_<config>_B<b>_<leg>_autotuned.json of the option-on legs")
    ap.add_argument("--no-drift", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_small_batch_time.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/f16_small_batch_time.py measures on the GPU"
    name, B = args.config, bench.DEFAULTS[args.config][0]
    config = bench.make_config(name)
    config.sampling.subsample = args.subsample
    config.device = "cuda:0"
    net = HipScoreNet(config)
    net.load_state_dict(synthetic.random_state_dict(net, seed=123), strict=True)
    x, cond = synthetic.random_inputs(config, 0, B)
    x, cond = x.cuda(), cond.cuda()
    nfr, nfp = config.data.num_frames, config.sampling.num_frames_pred

    def call(seed):
        if nfp > nfr:
            g = torch.Generator(device="cuda").manual_seed(seed)
            return video_gen(config, net, cond, num_frames_pred=nfp, seed=seed, init_noise_fn=lambda k, shp, dev: torch.randn(shp, device=dev, generator=g))
        return ddpm_sampler(x, net, cond=cond, final_only=True, denoise=True, subsample_steps=args.subsample, clip_before=True, verbose=False,
                            log=False, seed=seed)[0]

    lines = [f"\n# tools/f16_small_batch_time.py [{args.label}]: {name}, B = {B}, DDPM-{args.subsample} + denoise, {B * nfp} frames per call, "
             f"{torch.cuda.get_device_name(0)}; {args.rounds} alternating rounds of {args.calls} timed call(s) per leg (one warm-up call each); every leg "
             "autotuned in this process"]

    tables, fps, ids = {}, {k: [] for k, _ in LEGS}, {}
    for r in range(args.rounds):
        for leg, opts in LEGS:
            for k, v in opts.items():
                net.set_option(k, v)
            if leg in tables:
                net.set_tuning(B, tables[leg])
            call(999)                                            # warm-up (first round: the autotune)
            tables[leg] = net.get_tuning(B)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.calls):
                call(1000 + i)
            torch.cuda.synchronize()
            fps[leg].append(args.calls * B * nfp / (time.perf_counter() - t0))
            ids[leg] = conv3_ids(net)
    mean = {leg: sum(v) / len(v) for leg, v in fps.items()}
    lines.append("## frames/s: mean of the rounds [each round] spread = (max - min) / mean; x of the default leg; 3x3 conv ops per kernel id")
    for leg, _ in LEGS:
        v = fps[leg]
        lines.append(f"{leg:8s} {mean[leg]:8.2f} frames/s  [{', '.join(f'{q:.2f}' for q in v)}]  spread {100 * (max(v) - min(v)) / mean[leg]:.2f} %   "
                     f"x{mean[leg] / mean['default']:.3f}   ids {ids[leg]}")
    k4 = {leg: {k: c for k, c in ids[leg].items() if k in (26, 27)} for leg, _ in LEGS}
    lines.append(f"the 4-way K split of the fp16 kernels (ids 26 / 27) was chosen for: {k4}")
    if args.save_tables:
        os.makedirs(args.save_tables, exist_ok=True)
        for leg in ("f16x2", "f16x1", "both"):
            import json
            json.dump({str(B): tables[leg]}, open(os.path.join(args.save_tables, f"tune_{name}_B{B}_{leg}_autotuned.json"), "w"))
    # ---- the default arithmetic under the committed table: the same bits from every build
    if args.frames:
        net.set_option("f16x2", 0)
        net.set_option("f16x1", 0)
        net.load_tuning(os.path.join(ROOT, "profiles", f"tune_{name}_B{B}_bf16x3.json"))
        fr = call(4242).cpu()
        if os.path.exists(args.frames):
            other = torch.load(args.frames)
            same = torch.equal(fr, other)
            lines.append(f"default arithmetic, committed table, seed 4242: frames torch.equal to {os.path.basename(args.frames)}: {same}"
                         + ("" if same else f" (max-abs difference {(fr - other).abs().max().item():.3e})"))
        else:
            os.makedirs(os.path.dirname(os.path.abspath(args.frames)), exist_ok=True)
            torch.save(fr, args.frames)
            lines.append(f"default arithmetic, committed table, seed 4242: frames written to {os.path.basename(args.frames)}")
    del net
    if name == "bair_big_spade" and not args.no_drift:
        drift_config4(lines)
    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "a").write(txt)


if __name__ == "__main__":
    main()
