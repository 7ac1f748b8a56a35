"""The ngf-288 UCF-101 net (configs/ucf101.yml with the sampling scripts' overrides model.ngf = 288, model.n_head_channels = 288: ch_mult [1, 2, 3, 4],
4 + 4 frames of 3 channels at 64 x 64) on one MI355X, one process: profiles/w288_time.txt.

    python tools/w288_time.py --layers [--batches 8 60] [--reps 20] [--out profiles/w288_time.txt]
    python tools/w288_time.py --e2e [--batch 8] [--out ...]

Synthetic weights and inputs (bench.py's).  The up path of this net opens with two blocks over a 1152 + 1152 = 2304-channel concat at 8 x 8: a 3x3 conv
2304 -> 1152 behind GroupNorm + SiLU and a 1x1 shortcut 2304 -> 1152 over the raw concat, each.
(a) --layers: per batch size one autotuned sampler call (the tuner's table), then one table per candidate that differs from the tuner's in those four
    ops only; per table `reps` one-step sampler calls under the option "profile" (HIP events round every op of the call's first forward).  Per op and
    candidate: the median of the `reps` times and the kernel that ran.  3x3: the direct tiles 0-3 with every cout tile of 32 .. 128 channels (what a
    2304-channel layer ran before ids 18 / 19 / 26 / 27 took it; the best one is the baseline), 18 / 19, 26 under f16x2, 27 under f16x1.  1x1: the
    direct tiles, dma1 (5 / 6 / 9) and the split-operand GEMM 15 (14 under f16x2) at every cout tile they take.
(b) --e2e: DDPM with subsample_steps = 10 + denoise, frames/s (B * 4 frames per call), default / f16x2 / f16x1, every leg autotuned; and the same legs
    with the two 2304-channel 3x3 layers pinned to their best direct tile through the tuning table (this net does not load on the previous commit:
    that is the baseline).  Device memory after load is recorded.
Needs a GPU; reads nothing outside the repository.
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
from tools.wide_conv_time import NAMES, inputs, one_step, profile  # noqa: E402

NAMES = {**NAMES, 5: "dma1", 6: "dma1_ck32", 9: "dma1_px64", 14: "gemm1_f16x2", 15: "gemm1_bf16x3"}
TILES = [(k, c) for k in (0, 1, 2, 3) for c in (1, 2, 3, 4)]


def make_net():
    config = bench.make_config("smmnist_big5_ngf96")
    config.data.channels = 3
    config.data.num_frames = 4
    config.data.num_frames_cond = 4
    config.model.ngf = 288
    config.model.n_head_channels = 288
    config.device = "cuda:0"
    free0, total = torch.cuda.mem_get_info()
    net = HipScoreNet(config)
    net.load_state_dict(synthetic.random_state_dict(net, seed=123), strict=True)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    return config, net, (free0 - free1) / 2 ** 20


def is_2304(op):
    return op[1] == 3 and op[4] == 2304


def time_tables(net, B, x, cond, table0, ops, cands, reps):
    """{(op index, id, cout tile): (median ms, kernel that ran)} with `ops` moved to each (id, cout tile) of `cands` in turn."""
    res = {}
    for kid, cot in cands:
        table = [list(e) for e in table0]
        for op in ops:
            table[op[0]] = [kid, cot if cot and op[5] % (32 * cot) == 0 else (1 if cot else 0)]
        net.set_tuning(B, table)
        one_step(net, x, cond)
        samples, ran = {op[0]: [] for op in ops}, {}
        for r in range(reps):
            one_step(net, x, cond, seed=2 + r)
            for op in profile(net):
                if op[0] in samples:
                    samples[op[0]].append(op[6])
                    ran[op[0]] = op[7]
        for op in ops:
            res[(op[0], kid, cot)] = (statistics.median(samples[op[0]]), ran[op[0]])
    net.set_tuning(B, table0)
    return res


def best_of(res, i, ids, must_run=True):
    """(ms, id, cout tile) of the fastest candidate of `ids` for op i that ran the id it names (a refused one fell back to a tile)."""
    c = [(v[0], k[1], k[2]) for k, v in res.items() if k[0] == i and k[1] in ids and (not must_run or v[1] == k[1] or (k[1] <= 3 and v[1] <= 3))]
    return min(c) if c else None


def layers(lines, batches, reps):
    config, net, mb = make_net()
    lines.append(f"device memory after load (default arithmetic, before the first forward): {mb:.0f} MiB")
    net.set_option("profile", 1)
    for B in batches:
        x, cond = inputs(config, B)
        picks, res = {}, {}
        for opt in (None, "f16x2", "f16x1"):
            if opt:
                net.set_option(opt, 1)
            one_step(net, x, cond)                              # autotunes
            tab = net.get_tuning(B)
            picks[opt] = {op[0]: (op[7], tab[op[0]][1], op[6]) for op in profile(net) if is_2304(op)}
            if opt is None:
                table0 = tab
                wide = [op for op in profile(net) if is_2304(op)]
                w3, w1 = [op for op in wide if op[2] == 3], [op for op in wide if op[2] == 1]
                res.update(time_tables(net, B, x, cond, table0, wide, TILES, reps))
                res.update(time_tables(net, B, x, cond, table0, w3, [(18, 0), (19, 0)], reps))
                res.update(time_tables(net, B, x, cond, table0, w1, [(k, c) for k in (5, 6, 9, 15) for c in (1, 2, 3, 4)], reps))
            elif opt == "f16x2":
                res.update(time_tables(net, B, x, cond, tab, w3, [(26, 0)], reps))
                res.update(time_tables(net, B, x, cond, tab, w1, [(14, c) for c in (1, 2, 3, 4)], reps))
            else:
                res.update(time_tables(net, B, x, cond, tab, w3, [(27, 0)], reps))
            if opt:
                net.set_option(opt, 0)
        mark = len(lines)
        lines.append(f"## (a) B = {B}: the ops over the 2304-channel concat at 8 x 8, us, median of {reps} forwards [kernel that ran]")
        for op in wide:
            i, _, ks, H, Cin, Cout = op[:6]
            fl = 2.0 * ks * ks * Cin * Cout * H * H * B
            tile = best_of(res, i, (0, 1, 2, 3))
            lines.append(f"op {i:3d} {ks}x{ks} {H}x{H} {Cin} -> {Cout}: best direct tile {tile[0] * 1e3:.1f} us ({fl / tile[0] * 1e-9:.1f} TFLOP/s direct form) "
                         f"[{NAMES[tile[1]]}, cout tile {32 * tile[2]}]")
            for (j, kid, cot), (ms, ran) in sorted(res.items()):
                if j != i or kid <= 3:
                    continue
                took = ran == kid
                lines.append(f"        id {kid:2d}" + (f" cout tile {32 * cot:3d}" if cot else "") + (f": {ms * 1e3:8.1f} us  x{tile[0] / ms:.2f} of the best tile"
                             if took else f": refused (ran {NAMES.get(ran, ran)})") + (f" [{NAMES.get(ran, ran)}]" if took else ""))
            lines.append("        the tuner picked " + ", ".join(f"{opt or 'default'}: {NAMES.get(picks[opt][i][0], picks[opt][i][0])}"
                         + (f" cout tile {32 * picks[opt][i][1]}" if ks == 1 or picks[opt][i][0] <= 3 else "") + f" ({picks[opt][i][2] * 1e3:.1f} us)" for opt in picks))
        print("\n".join(lines[mark:]), flush=True)
    del net


def e2e(lines, rounds, calls, B):
    sub = 10
    config, net, mb = make_net()
    x, cond = inputs(config, B)
    lines.append(f"## (b) end to end: B = {B}, DDPM-{sub} + denoise, frames/s = B * {config.data.num_frames} frames / call; {rounds} rounds of {calls} timed calls behind "
                 f"one warm-up call (the first one autotunes); device memory after load {mb:.0f} MiB")

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
        for label in ("tuned", "2304-channel 3x3 layers pinned to their best direct tile"):
            if label != "tuned":
                w3 = [op for op in forward_profile() if is_2304(op) and op[2] == 3]
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
            wide = [op for op in ops if is_2304(op)]
            lines.append(f"{opt or 'default':8s} {label}: {sum(fps) / rounds:9.2f} frames/s  [{', '.join(f'{q:.2f}' for q in fps)}]   one forward {total:.3f} ms; "
                         + ", ".join(f"{op[2]}x{op[2]} {op[4]}->{op[5]} {op[6] * 1e3:.0f} us [{NAMES.get(op[7], op[7])}]" for op in wide))
            print(lines[-1], flush=True)
        net.set_tuning(B, tuned)
        if opt:
            net.set_option(opt, 0)
    free, total = torch.cuda.mem_get_info()
    lines.append(f"device memory in use at the end (all three arithmetics' weight images, workspace at B = {B}): {(total - free) / 2 ** 20:.0f} MiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--batch", type=int, default=8, help="--e2e: the batch size")
    ap.add_argument("--batches", type=int, nargs="*", default=[8, 60])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w288_time.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/w288_time.py measures on the GPU"
    lines = [f"# tools/w288_time.py: {torch.cuda.get_device_name(0)}, one process, library {os.path.basename(_lib.LIB_PATH)}"]
    if args.layers:
        layers(lines, args.batches, args.reps)
    if args.e2e:
        e2e(lines, args.rounds, args.calls, args.batch)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "a").write("\n".join(lines) + "\n")
    print("appended to:", args.out)


if __name__ == "__main__":
    main()
