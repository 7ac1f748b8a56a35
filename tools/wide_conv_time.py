"""The 3x3 layers of more than 1024 input channels of the UCF-101 net (configs/ucf101.yml: ngf 192, ch_mult [1, 2, 3, 4], 64 x 64) on the K-split
Winograd kernels against the direct tile kernels that ran them before, one process on one MI355X: profiles/wide_conv_time.txt.

    python tools/wide_conv_time.py --layers [--batches 8 64] [--reps 20] [--out profiles/wide_conv_time.txt]
    python tools/wide_conv_time.py --e2e [--label new] [--net cityscapes_big_spade --batch 2] [--out ...]
                                                                  (MCVD_LIB_PATH=<a build of the previous commit>: the "before" leg)

The net: BASELINE config 2's data block with channels = 3, num_frames = 4, num_frames_cond = 4; model.ngf = 192, n_head_channels = 96; synthetic
weights and inputs (bench.py's).  Its up path holds five 3x3 convs above 1024 channels -- 8 x 8: 1536 -> 768 (x2), 1344 -> 768; 16 x 16: 1344 -> 576,
1152 -> 576 -- each behind a GroupNorm + SiLU over a virtual concat.
(a) --layers: per batch size, one autotuned sampler call (the tuner's table), then one table per kernel id that differs from the tuner's in the five
    layers only; per table `reps` sampler calls of one step under the option "profile", which brackets every op of the call's first forward with HIP
    events.  Per layer and id: the median of the `reps` times, the direct-form TFLOP/s (2 * 9 * Cin * Cout * H * W * B / time), the kernel that ran.
    Ids 0-3 are the direct tiles (what ran before; timed with every cout tile of 32 .. 128 channels the layer divides by, the best one reported),
    8 / 11 / 18 / 19 the fp32 and three-piece bf16 K splits, 13 / 26 under f16x2, 25 / 27 under f16x1.
(b) --e2e: DDPM with subsample_steps = 10 + denoise at B = 8, frames/s (B * 4 frames per call), under the default arithmetic, f16x2 and f16x1; and
    the share of one forward the five layers hold (per-op times of the same "profile" option).
Needs a GPU; reads nothing outside the repository.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from mcvd_pytorch_amd import HipScoreNet, _lib, ddpm_sampler, synthetic  # noqa: E402

DEFAULT_IDS = [0, 1, 2, 3, 8, 11, 18, 19]
NAMES = {0: "tile256", 1: "tile128", 2: "tile64", 3: "tile64_splitk", 4: "wino", 8: "wino_k2", 10: "wino3", 11: "wino3_k2", 13: "wino2h_k2", 18: "wino3_k4",
         19: "wino3_k8", 25: "wino1h_k2", 26: "wino2h_k4", 27: "wino1h_k4", 12: "wino2h", 24: "wino1h", 16: "wino3p", 17: "wino3p_k2", 20: "wino3p_k4"}


def make_net(name="ucf101"):
    if name == "ucf101":
        config = bench.make_config("smmnist_big5_ngf96")
        config.data.channels = 3
        config.data.num_frames = 4
        config.data.num_frames_cond = 4
        config.model.ngf = 192
        config.model.n_head_channels = 96
    else:                                          # configs/cityscapes_big_spade.yml: 128 x 128, ch_mult [1, 1, 2, 3, 4], the same five layers behind SPADE norms
        assert name == "cityscapes_big_spade", name
        config = bench.make_config("cityscapes_big")
        config.model.ngf = 192
        config.model.n_head_channels = 192
        config.model.spade = True
        config.model.spade_dim = 256
    config.device = "cuda:0"
    net = HipScoreNet(config)
    net.load_state_dict(synthetic.random_state_dict(net, seed=123), strict=True)
    return config, net


def inputs(config, B):
    x, cond = synthetic.random_inputs(config, 0, B)
    return x.cuda(), cond.cuda()


def profile(net):
    """[(op index, kind, ks, H, Cin, Cout, ms, kernel that ran)] of the last sampler call's first forward."""
    n = _lib.lib.mcvd_model_profile_read(net._model, None, None, None, None, None, 0)
    kinds, kss = (C.c_int * n)(), (C.c_int * n)()
    ms, fl, by = (C.c_double * n)(), (C.c_double * n)(), (C.c_double * n)()
    assert _lib.lib.mcvd_model_profile_read(net._model, kinds, kss, ms, fl, by, n) == n
    info, out = (C.c_int * 8)(), []
    for i in range(n):
        _lib.check(_lib.lib.mcvd_model_op_info(net._model, i, info), "op_info")
        out.append((i, kinds[i], info[2], info[3], info[4], info[5], ms[i], _lib.lib.mcvd_model_op_kernel(net._model, i) if kinds[i] == 3 else -1))
    return out


def is_wide(op):
    return op[1] == 3 and op[2] == 3 and op[4] > 1024


def one_step(net, x, cond, seed=1):
    ddpm_sampler(x, net, cond=cond, final_only=True, denoise=False, subsample_steps=1, clip_before=True, verbose=False, log=False, seed=seed)
    torch.cuda.synchronize()


def layers(lines, batches, reps):
    config, net = make_net()
    net.set_option("profile", 1)
    for B in batches:
        x, cond = inputs(config, B)
        picks = {}
        for opt in (None, "f16x2", "f16x1"):                   # the tuner's own choice under each arithmetic
            if opt:
                net.set_option(opt, 1)
            one_step(net, x, cond)
            table = net.get_tuning(B)
            picks[opt] = {op[0]: (op[7], op[6]) for op in profile(net) if is_wide(op)}
            if opt is None:
                table0, wide = table, [op for op in profile(net) if is_wide(op)]
            if opt:
                net.set_option(opt, 0)
        lines.append(f"## (a) B = {B}: the five layers, us (direct-form TFLOP/s) [kernel that ran], median of {reps} forwards; the tuner's pick per arithmetic")
        res = {}
        for opt, ids in ((None, DEFAULT_IDS), ("f16x2", [13, 26]), ("f16x1", [25, 27])):
            if opt:
                net.set_option(opt, 1)
            # the direct tiles take a cout tile of 1 .. 4 x 32 channels (the tuner times two of them): each is timed, the best one is reported
            for kid, cot in [(k, c) for k in ids for c in ((1, 2, 3, 4) if k <= 3 else (0,))]:
                table = [list(e) for e in table0]
                for op in wide:
                    table[op[0]] = [kid, cot if op[5] % (32 * max(cot, 1)) == 0 else 1]
                net.set_tuning(B, table)
                one_step(net, x, cond)                          # warm-up
                samples = {op[0]: [] for op in wide}
                ran = {}
                for r in range(reps):
                    one_step(net, x, cond, seed=2 + r)
                    for op in profile(net):
                        if op[0] in samples:
                            samples[op[0]].append(op[6])
                            ran[op[0]] = op[7]
                for op in wide:
                    cand = (statistics.median(samples[op[0]]), ran[op[0]], cot)
                    if (op[0], kid) not in res or cand[0] < res[(op[0], kid)][0]:
                        res[(op[0], kid)] = cand
            if opt:
                net.set_option(opt, 0)
        net.set_tuning(B, table0)
        for op in wide:
            i, _, _, H, Cin, Cout, _, _ = op
            fl = 2.0 * 9 * Cin * Cout * H * H * B
            cells = []
            for kid in DEFAULT_IDS + [13, 26, 25, 27]:
                ms, ran, cot = res[(i, kid)]
                cells.append(f"{kid}: {ms * 1e3:8.1f} us ({fl / ms * 1e-9:6.1f}) [{NAMES.get(ran, ran)}" + (f", cout tile {32 * cot}]" if cot else "]"))
            tile = min(res[(i, k)][0] for k in (0, 1, 2, 3))
            best3 = min(res[(i, k)][0] for k in (11, 18, 19))
            lines.append(f"op {i:3d} {H:2d}x{H:<2d} {Cin:4d} -> {Cout:3d} | " + " | ".join(cells))
            lines.append(f"        best tile {tile * 1e3:.1f} us, best bf16x3 K split {best3 * 1e3:.1f} us: x{tile / best3:.2f}; tuner picked "
                         + ", ".join(f"{opt or 'default'}: {NAMES.get(picks[opt][i][0], picks[opt][i][0])} ({picks[opt][i][1] * 1e3:.1f} us)" for opt in picks))
            print(lines[-2], flush=True)
            print(lines[-1], flush=True)
    del net


def e2e(lines, label, rounds, calls, name, B):
    sub = 10
    config, net = make_net(name)
    x, cond = inputs(config, B)
    lines.append(f"## (b) end to end [{label}], {name}: B = {B}, DDPM-{sub} + denoise, frames/s = B * {config.data.num_frames} frames / call; {rounds} rounds of {calls} timed "
                 "calls behind one warm-up call (the first one autotunes)")
    for opt in (None, "f16x2", "f16x1"):
        if opt:
            net.set_option(opt, 1)
        fps = []
        for r in range(rounds):
            def call(seed):
                return ddpm_sampler(x, net, cond=cond, final_only=True, denoise=True, subsample_steps=sub, clip_before=True, verbose=False, log=False, seed=seed)[0]
            call(999)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(calls):
                call(1000 + i)
            torch.cuda.synchronize()
            fps.append(calls * B * config.data.num_frames / (time.perf_counter() - t0))
        net.set_option("profile", 1)
        one_step(net, x, cond)
        one_step(net, x, cond)
        ops = profile(net)
        net.set_option("profile", 0)
        total = sum(op[6] for op in ops)
        wide = [op for op in ops if is_wide(op)]
        share = sum(op[6] for op in wide)
        lines.append(f"{label:6s} {opt or 'default':8s} {sum(fps) / rounds:9.2f} frames/s  [{', '.join(f'{q:.2f}' for q in fps)}]   one forward {total:.3f} ms, the five layers "
                     f"{share:.3f} ms = {100 * share / total:.1f} %: " + ", ".join(f"{op[3]}x{op[3]} {op[4]}->{op[5]} {op[6] * 1e3:.0f} us [{NAMES.get(op[7], op[7])}]" for op in wide))
        print(lines[-1], flush=True)
        if opt:
            net.set_option(opt, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--label", default="new")
    ap.add_argument("--net", default="ucf101", choices=["ucf101", "cityscapes_big_spade"], help="--e2e: the net")
    ap.add_argument("--batch", type=int, default=8, help="--e2e: the batch size")
    ap.add_argument("--batches", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_conv_time.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/wide_conv_time.py measures on the GPU"
    lines = [f"# tools/wide_conv_time.py: {torch.cuda.get_device_name(0)}, one process, library {os.path.basename(_lib.LIB_PATH)}"]
    if args.layers:
        layers(lines, args.batches, args.reps)
    if args.e2e:
        e2e(lines, args.label, args.rounds, args.calls, args.net, args.batch)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "a").write("\n".join(lines) + "\n")
    print("appended to:", args.out)


if __name__ == "__main__":
    main()
