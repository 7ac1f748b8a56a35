"""What the one-piece fp16 arithmetic ("f16x1") buys, measured in ONE process on one MI355X: profiles/f16x1_time.txt.

    python tools/f16x1_time.py [--batch 64] [--steps 2] [--rounds 2] [--second-legs] [--out profiles/f16x1_time.txt]

Workload: BASELINE config 2 (smmnist_big5_ngf96), DDPM-100 + denoise, the bench's batch, weights and inputs.
  * frames/s under default, f16x2, f16x1 and f16x1 + f16x2.  default / f16x2 run the committed kernel tables bench.py pins
    (profiles/tune_smmnist_big5_ngf96_B64_{bf16x3,f16x2}.json), the two f16x1 legs a table autotuned in this run.  The legs ALTERNATE over
    `rounds` rounds (one warm-up call, then `steps` timed sampler calls between device synchronisations, each round); every ratio is
    against the default / f16x2 figure of the same run: boxes differ by +- 4 %, earlier records are no baseline.
  * average launch time of shape ids 10, 16, 12 and 24 over config 2's GroupNorm-ed 3x3 layers: every 3x3 conv forced onto the id
    (conv_shape), one profiled forward (HIP events around every op, mcvd_model_profile_read), averaged over the layers that id really
    took in all four runs.
  * the share of uint8 pixels (inverse_data_transform + mcvd_pack_frames_u8) that differ from the default run's, same seeds.
  * --second-legs (a run of its own, APPENDED to the file): frames/s of configs 4 (bair_big_spade) and 5 (cityscapes_big) under default
    and f16x1 (autotuned both), at `--second-subsample` sampler steps.
Needs a GPU; nothing here falls back.
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
from mcvd_pytorch_amd.runner import frames_to_uint8, inverse_data_transform  # noqa: E402

LEGS = [("default", dict(f16x2=0, f16x1=0), "bf16x3"), ("f16x2", dict(f16x2=1, f16x1=0), "f16x2"),
        ("f16x1", dict(f16x2=0, f16x1=1), None), ("f16x1+f16x2", dict(f16x2=1, f16x1=1), None)]


def make(name, B, subsample=None):
    config = bench.make_config(name)
    if subsample:
        config.sampling.subsample = subsample
    config.device = "cuda:0"
    net = HipScoreNet(config)
    net.load_state_dict(synthetic.random_state_dict(net, seed=123), strict=True)
    x, cond = synthetic.random_inputs(config, 0, B)
    return config, net, x.cuda(), cond.cuda()


def conv_ops(net):
    """[(op index, ks, kernel that ran, normed input, ms of the profiled forward)]"""
    n = _lib.lib.mcvd_model_profile_read(net._model, None, None, None, None, None, 0)
    kinds, kss = (C.c_int * n)(), (C.c_int * n)()
    ms, fl, by = (C.c_double * n)(), (C.c_double * n)(), (C.c_double * n)()
    _lib.check(0 if _lib.lib.mcvd_model_profile_read(net._model, kinds, kss, ms, fl, by, n) == n else -1, "profile_read")
    info, out = (C.c_int * 8)(), []
    for i in range(n):
        _lib.check(_lib.lib.mcvd_model_op_info(net._model, i, info), "op_info")
        if info[0] == 3:
            out.append((i, info[2], _lib.lib.mcvd_model_op_kernel(net._model, i), bool(info[7]), ms[i]))
    return out


def second_legs(args):
    lines = [f"\n## second legs ({torch.cuda.get_device_name(0)}): default vs f16x1 (both autotuned in this run), DDPM-{args.second_subsample}, "
             f"{args.rounds} alternating rounds of one timed call"]
    for name2 in ("bair_big_spade", "cityscapes_big"):
        B2 = bench.DEFAULTS[name2][0]
        config2, net2, x2, cond2 = make(name2, B2, args.second_subsample)
        nfr, nfp2 = config2.data.num_frames, config2.sampling.num_frames_pred

        def call2(seed):
            if nfp2 > nfr:
                g = torch.Generator(device="cuda").manual_seed(seed)
                return video_gen(config2, net2, cond2, num_frames_pred=nfp2, seed=seed, init_noise_fn=lambda k, shp, dev: torch.randn(shp, device=dev, generator=g))
            return ddpm_sampler(x2, net2, cond=cond2, final_only=True, denoise=True, subsample_steps=args.second_subsample, clip_before=True,
                                verbose=False, log=False, seed=seed)[0]
        res, tab = {"default": [], "f16x1": []}, {}
        for r in range(args.rounds):
            for leg in res:
                net2.set_option("f16x1", 1 if leg == "f16x1" else 0)
                if leg in tab:
                    net2.set_tuning(B2, tab[leg])
                call2(5)
                tab[leg] = net2.get_tuning(B2)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call2(6)
                torch.cuda.synchronize()
                res[leg].append(B2 * nfp2 / (time.perf_counter() - t0))
        m = {k: sum(v) / len(v) for k, v in res.items()}
        lines.append(f"{name2:16s} B = {B2}: default {m['default']:.1f} frames/s {[round(v, 1) for v in res['default']]}, f16x1 {m['f16x1']:.1f} frames/s "
                     f"{[round(v, 1) for v in res['f16x1']]}: x{m['f16x1'] / m['default']:.3f}")
        del net2
    txt = "\n".join(lines) + "\n"
    print(txt)
    open(args.out, "a").write(txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--second-legs", action="store_true")
    ap.add_argument("--second-subsample", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16x1_time.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/f16x1_time.py measures on the GPU"
    if args.second_legs:
        return second_legs(args)
    B, name = args.batch, "smmnist_big5_ngf96"
    config, net, x, cond = make(name, B)
    sub = bench.DEFAULTS[name][1]
    nfp = config.sampling.num_frames_pred
    lines = [f"# tools/f16x1_time.py: {name}, B = {B}, DDPM-{sub} + denoise, {torch.cuda.get_device_name(0)}; {args.rounds} alternating rounds of {args.steps} timed "
             f"sampler calls per leg (one warm-up call each); all figures from this one process"]

    def call(seed):
        return ddpm_sampler(x, net, cond=cond, final_only=True, denoise=True, subsample_steps=sub, clip_before=True, verbose=False, log=False, seed=seed)[0]

    tables, fps, frames, kernels = {}, {k: [] for k, _, _ in LEGS}, {}, {}
    for r in range(args.rounds):
        for leg, opts, pinned in LEGS:
            for k, v in opts.items():
                net.set_option(k, v)
            if pinned and B == 64:
                net.load_tuning(os.path.join(ROOT, "profiles", f"tune_{name}_B64_{pinned}.json"))
            elif leg in tables:
                net.set_tuning(B, tables[leg])
            net.set_option("profile", 1)
            call(999)                                            # warm-up (and, for the f16x1 legs' first round, the autotune)
            tables[leg] = net.get_tuning(B)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                out = call(1000 + i)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            fps[leg].append(args.steps * B * nfp / dt)
            frames[leg] = out
            ran = [k for _, ks, k, _, _ in conv_ops(net) if ks == 3]
            kernels[leg] = {k: ran.count(k) for k in sorted(set(ran))}
    base = {leg: sum(v) / len(v) for leg, v in fps.items()}
    lines.append("\n## frames/s (mean of the rounds; each round's figure in brackets); 3x3 conv ops per kernel id")
    for leg, _, pinned in LEGS:
        lines.append(f"{leg:12s} {base[leg]:8.1f} frames/s  [{', '.join(f'{v:.1f}' for v in fps[leg])}]   x{base[leg] / base['default']:.3f} of default, "
                     f"x{base[leg] / base['f16x2']:.3f} of f16x2   table: {'committed ' + pinned if pinned and B == 64 else 'autotuned in this run'}   ids {kernels[leg]}")

    # ---- uint8 pixels that differ from the default run's (same seeds)
    lines.append("\n## uint8 pixels (inverse_data_transform + mcvd_pack_frames_u8) that differ from the default run's, last timed call")
    u8 = {leg: frames_to_uint8(net, inverse_data_transform(config, f), config.data.channels) for leg, f in frames.items()}
    for leg, _, _ in LEGS[1:]:
        diff = (u8[leg] != u8["default"])
        step = (u8[leg].int() - u8["default"].int()).abs().max().item()
        lines.append(f"{leg:12s} {100.0 * diff.float().mean().item():7.3f} % of {diff.numel()} pixels differ, by at most {step} grey level(s); "
                     f"max-abs frame difference {(frames[leg] - frames['default']).abs().max().item():.3e}")

    # ---- launch times per kernel id over the GroupNorm-ed 3x3 layers
    lines.append("\n## average launch time over config 2's GroupNorm-ed 3x3 layers, every 3x3 conv forced onto the id (one profiled forward, HIP events per op)")
    net.set_option("f16x2", 0)
    net.set_option("f16x1", 0)
    per_id = {}
    t = torch.full((B,), 500, dtype=torch.long, device="cuda")
    for kid in (10, 16, 12, 24):
        net.set_option("conv_shape", kid)
        net.set_option("profile", 1)
        net(x, t, cond=cond)                                     # warm-up: weight pieces packed, code objects loaded
        call(7)                                                  # the first forward of a sampler call is the profiled one
        torch.cuda.synchronize()
        per_id[kid] = {i: (k, ms) for i, ks, k, pro, ms in conv_ops(net) if ks == 3 and pro}
    net.set_option("conv_shape", -1)
    common = [i for i in per_id[24] if all(per_id[kid][i][0] in (kid, kid + 1) for kid in per_id)]
    for kid in per_id:
        v = [per_id[kid][i][1] for i in common]
        lines.append(f"id {kid:2d} (+ its K-split sibling where it applies): {1e3 * sum(v) / max(len(v), 1):8.1f} us average over {len(v)} layers, {sum(v):.3f} ms per forward")

    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(txt)


if __name__ == "__main__":
    main()
