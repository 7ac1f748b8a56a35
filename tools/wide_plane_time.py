"""The 32 x 32 3x3 layers above 1024 input channels of the ngf-288 UCF-101 net (tools/w288_time.py's net: ch_mult [1, 2, 3, 4], 4 + 4 frames of 3
channels at 64 x 64; the up path's 864 + 576 = 1440 -> 576 and 576 + 576 = 1152 -> 576) on the unsplit Winograd kernels against the direct tile
kernels that ran them before, one process on one MI355X: profiles/wide_plane_time.txt.

    python tools/wide_plane_time.py --layers [--batches 8 60] [--reps 20] [--out profiles/wide_plane_time.txt]
    python tools/wide_plane_time.py --e2e [--batch 8] [--out ...]

(a) --layers: per batch size one autotuned sampler call (the tuner's table), then one table per candidate that differs from the tuner's in those
    layers only; per table `reps` one-step sampler calls under the option "profile" (HIP events round every op of the call's first forward).  Per
    layer and candidate: the median of the `reps` times and the kernel that ran.  The direct tiles 0-3 with every cout tile of 32 .. 128 channels
    (what these layers ran before; the best one is the baseline), ids 10 / 4, 12 under f16x2, 24 under f16x1; the tuner's own pick per arithmetic.
    --also16 adds the 16 x 16 layers above 1024 channels, where the unsplit ids are new candidates beside the K splits (11 / 18, 13 / 26, 25 / 27).
(b) --e2e: DDPM with subsample_steps = 10 + denoise, frames/s (B * 4 frames per call), default / f16x2 / f16x1, every leg autotuned; and the same
    legs with the 32 x 32 layers pinned to their best direct tile through the tuning table: what the commit before ran.
Needs a GPU; reads nothing outside the repository.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mcvd_pytorch_amd import _lib, ddpm_sampler  # noqa: E402
from tools.w288_time import NAMES, TILES, best_of, make_net, time_tables  # noqa: E402
from tools.wide_conv_time import inputs, one_step, profile  # noqa: E402


def is_wide32(op):
    return op[1] == 3 and op[2] == 3 and op[3] == 32 and op[4] > 1024


def is_wide16(op):
    return op[1] == 3 and op[2] == 3 and op[3] == 16 and op[4] > 1024


def layers(lines, batches, reps, also16):
    config, net, mb = make_net()
    net.set_option("profile", 1)
    for B in batches:
        x, cond = inputs(config, B)
        picks, res = {}, {}
        sel = (lambda op: is_wide32(op) or is_wide16(op)) if also16 else is_wide32
        for opt, ids in ((None, [10, 4] + ([11, 18] if also16 else [])), ("f16x2", [12] + ([13, 26] if also16 else [])),
                         ("f16x1", [24] + ([25, 27] if also16 else []))):
            if opt:
                net.set_option(opt, 1)
            one_step(net, x, cond)                              # autotunes
            tab = net.get_tuning(B)
            picks[opt] = {op[0]: (op[7], tab[op[0]][1], op[6]) for op in profile(net) if sel(op)}
            if opt is None:
                table0 = tab
                wide = [op for op in profile(net) if sel(op)]
                res.update(time_tables(net, B, x, cond, table0, wide, TILES, reps))
            res.update(time_tables(net, B, x, cond, tab, wide, [(k, 0) for k in ids], reps))
            if opt:
                net.set_option(opt, 0)
        mark = len(lines)
        lines.append(f"## (a) B = {B}: the 3x3 layers above 1024 channels at 32 x 32" + (" and 16 x 16" if also16 else "") +
                     f", us, median of {reps} forwards [kernel that ran]")
        for op in wide:
            i, _, ks, H, Cin, Cout = op[:6]
            fl = 2.0 * 9 * Cin * Cout * H * H * B
            tile = best_of(res, i, (0, 1, 2, 3))
            lines.append(f"op {i:3d} 3x3 {H}x{H} {Cin} -> {Cout}: best direct tile {tile[0] * 1e3:.1f} us ({fl / tile[0] * 1e-9:.1f} TFLOP/s direct form) "
                         f"[{NAMES[tile[1]]}, cout tile {32 * tile[2]}]")
            for (j, kid, cot), (ms, ran) in sorted(res.items()):
                if j != i or kid <= 3:
                    continue
                lines.append(f"        id {kid:2d}" + (f": {ms * 1e3:8.1f} us  x{tile[0] / ms:.2f} of the best tile ({fl / ms * 1e-9:.1f} TFLOP/s direct form) [{NAMES.get(ran, ran)}]"
                             if ran == kid else f": refused (ran {NAMES.get(ran, ran)})"))
            lines.append("        the tuner picked " + ", ".join(f"{opt or 'default'}: {NAMES.get(picks[opt][i][0], picks[opt][i][0])}"
                         + (f" cout tile {32 * picks[opt][i][1]}" if picks[opt][i][0] <= 3 else "") + f" ({picks[opt][i][2] * 1e3:.1f} us)" for opt in picks))
        print("\n".join(lines[mark:]), flush=True)
    del net


def e2e(lines, rounds, calls, B):
    sub = 10
    config, net, mb = make_net()
    x, cond = inputs(config, B)
    lines.append(f"## (b) end to end: B = {B}, DDPM-{sub} + denoise, frames/s = B * {config.data.num_frames} frames / call; {rounds} rounds of {calls} timed calls behind "
                 "one warm-up call (the first one autotunes)")

    def call(seed):
        return ddpm_sampler(x, net, cond=cond, final_only=True, denoise=True, subsample_steps=sub, clip_before=True, verbose=False, log=False, seed=seed)[0]

    def fps_of():
        fps = []
        for r in range(rounds):
            call(999)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(calls):
                call(1000 + i)
            torch.cuda.synchronize()
            fps.append(calls * B * config.data.num_frames / (time.perf_counter() - t0))
        return fps

    def forward_profile():
        net.set_option("profile", 1)
        one_step(net, x, cond)
        one_step(net, x, cond)
        ops = profile(net)
        net.set_option("profile", 0)
        return ops
    for opt in (None, "f16x2", "f16x1"):
        if opt:
            net.set_option(opt, 1)
        call(998)                                               # autotunes this leg
        tuned = net.get_tuning(B)
        for label in ("tuned", "32 x 32 layers above 1024 channels pinned to their best direct tile"):
            if label != "tuned":
                w3 = [op for op in forward_profile() if is_wide32(op)]
                net.set_option("profile", 1)
                res = time_tables(net, B, x, cond, tuned, w3, TILES, 3)
                net.set_option("profile", 0)
                table = [list(e) for e in tuned]
                for op in w3:
                    _, kid, cot = best_of(res, op[0], (0, 1, 2, 3))
                    table[op[0]] = [kid, cot]
                net.set_tuning(B, table)
            fps = fps_of()
            ops = forward_profile()
            total = sum(op[6] for op in ops)
            wide = [op for op in ops if is_wide32(op)]
            lines.append(f"{opt or 'default':8s} {label}: {sum(fps) / rounds:9.2f} frames/s  [{', '.join(f'{q:.2f}' for q in fps)}]   one forward {total:.3f} ms; "
                         + ", ".join(f"{op[4]}->{op[5]} {op[6] * 1e3:.0f} us [{NAMES.get(op[7], op[7])}]" for op in wide))
            print(lines[-1], flush=True)
        net.set_tuning(B, tuned)
        if opt:
            net.set_option(opt, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--also16", action="store_true", help="--layers: the 16 x 16 layers above 1024 channels too")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--batch", type=int, default=8, help="--e2e: the batch size")
    ap.add_argument("--batches", type=int, nargs="*", default=[8, 60])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_plane_time.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/wide_plane_time.py measures on the GPU"
    lines = [f"# tools/wide_plane_time.py: {torch.cuda.get_device_name(0)}, one process, library {os.path.basename(_lib.LIB_PATH)}"]
    if args.layers:
        layers(lines, args.batches, args.reps, args.also16)
    if args.e2e:
        e2e(lines, args.rounds, args.calls, args.batch)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "a").write("\n".join(lines) + "\n")
    print("appended to:", args.out)


if __name__ == "__main__":
    main()
