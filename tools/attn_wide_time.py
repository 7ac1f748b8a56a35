"""The wide-head attention kernel (attention_wide.cpp, head dims 160 ... 1024) against what ran before it, one process on one MI355X:
profiles/attn_wide_time.txt.

    python tools/attn_wide_time.py [--reps 20] [--naive-limit 2.0] [--no-e2e] [--out profiles/attn_wide_time.txt]

(a) per op, through mcvd_op_attention: D in {160, 192, 224, 256, 288, 384, 512, 768, 1024} x HW in {64, 256, 1024}, one head, B = 64
    (B * heads = 64), randn inputs; option naive_attn = 1 (one thread per query), 2 (the dispatch before the wide kernel: fp32 flash kernel up
    to D = 256, one thread per query beyond -- there the naive_attn = 1 figure is the same kernel and is not measured twice), 0 (the table's
    choice), 3 (two fp16 pieces), and 4 / 2 forced on 160 ... 256 where the table has to choose between the wide and the fp32 flash kernel.
    HIP events around every launch, 3 warm-up launches, median of `reps` >= 20.  The one-thread-per-query leg is slow: it is warmed up by ONE
    launch, that launch is timed, and the repeat count is capped so that the timed launches of a shape fit `naive-limit` seconds (at least
    one); the count is reported.  Direct-form TFLOP/s = 4 HW^2 D per head / time.
(b) end to end: BASELINE config 2 (smmnist_big5_ngf96) with model.n_head_channels = -1 -- single heads of 192 / 288 / 384 channels at
    32 x 32 / 16 x 16 / 8 x 8 -- B = 8, DDPM with subsample_steps = 10 + denoise, frames/s with naive_attn = 2 and 0; beside them the stock
    96-channel-head config 2 at the same B.  Synthetic weights and inputs (bench.py's).  Needs a GPU; reads nothing outside the repository.
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
from tests.hiputil import Ctx  # noqa: E402

DIMS = [160, 192, 224, 256, 288, 384, 512, 768, 1024]
HWS = [64, 256, 1024]
BH = 64
NAMES = {0: "naive", 1: "flash_f32", 2: "split2", 3: "split3", 4: "split3_presplit", 5: "wide2", 6: "wide3"}


def timed(ctx, qkv, reps, warm):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for _ in range(warm):
        ctx.attention(qkv, 1)
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        ctx.attention(qkv, 1)
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev), _lib.lib.mcvd_last_attention_kernel()


def leg(ctx, qkv, mode, f16x2, reps, warm=3):
    ctx.opt("f16x2", f16x2)
    ctx.opt("naive_attn", mode)
    try:
        return timed(ctx, qkv, reps, warm)
    finally:
        ctx.opt("naive_attn", 0)
        ctx.opt("f16x2", 0)


def per_op(lines, reps, naive_limit):
    ctx = Ctx()
    lines.append(f"## (a) per op: mcvd_op_attention, B = {BH}, one head, randn; ms (direct-form TFLOP/s) [kernel that ran]; median of {reps} launches, "
                 "the one-thread-per-query leg as noted")
    lines.append("#   D    HW | naive_attn=1 (launches timed)   | naive_attn=2 = before        | naive_attn=0 = the table      | naive_attn=3 (f16x2)          "
                 "| before / table | 160..256: wide3 forced (4) vs fp32 flash (2)")
    worst = {}
    for D in DIMS:
        for HW in HWS:
            qkv = torch.randn(BH, 3 * D, HW, device="cuda")
            fl = 4.0 * HW * HW * D * BH

            def fmt(ms, k):
                return f"{ms:10.4f} ms ({fl / ms * 1e-9:7.2f}) [{NAMES[k]}]"
            # one thread per query: one launch as warm-up AND first sample, then as many as fit the limit
            ctx.opt("naive_attn", 1)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record(); ctx.attention(qkv, 1); b.record()
            torch.cuda.synchronize()
            first, wall = a.elapsed_time(b), time.perf_counter() - t0
            n = max(1, min(reps, int(naive_limit * 1e3 / max(first, 1e-3))))
            naive_ms, k1 = leg(ctx, qkv, 1, 0, n, warm=0)
            ctx.opt("naive_attn", 0)
            if D <= 256:
                before_ms, k2 = leg(ctx, qkv, 2, 0, reps)
            else:
                before_ms, k2 = naive_ms, k1                   # the same kernel on the same input
            table_ms, k0 = leg(ctx, qkv, 0, 0, reps)
            f16_ms, k3 = leg(ctx, qkv, 3, 0, reps)
            extra = ""
            if D <= 256:
                w_ms, kw = leg(ctx, qkv, 4, 0, reps)
                extra = f" | wide3 {w_ms:.4f} ms vs flash_f32 {before_ms:.4f} ms: x{before_ms / w_ms:.2f}" if kw == 6 else f" | (4 ran {NAMES[kw]})"
            ratio = before_ms / table_ms
            worst[(D, HW)] = ratio
            lines.append(f"{D:5d} {HW:5d} | {fmt(naive_ms, k1)} ({n:2d}; first launch {first:.1f} ms, {wall:.2f} s wall) | {fmt(before_ms, k2)} | {fmt(table_ms, k0)} | "
                         f"{fmt(f16_ms, k3)} | x{ratio:9.2f}{extra}")
            print(lines[-1], flush=True)
    slower = {k: v for k, v in worst.items() if v < 1.0}
    lines.append(f"the table's kernel is slower than what ran before at: {slower if slower else 'no measured (D, HW)'}")
    lines.append("before / table for D > 256 (one thread per query -> wide3): " + ", ".join(f"D{d} HW{h} x{worst[(d, h)]:.1f}" for d in DIMS if d > 256 for h in HWS))
    del ctx


def e2e(lines, rounds, calls):
    B, sub = 8, 10
    lines.append(f"## (b) end to end: smmnist_big5_ngf96 (BASELINE config 2), B = {B}, DDPM-{sub} + denoise, frames/s = B * 5 frames / call; {rounds} alternating "
                 f"rounds of {calls} timed calls (one warm-up call each; the first warm-up autotunes the convs)")
    nets = {}
    for name, nhc in (("n_head_channels=-1", -1), ("stock (96-channel heads)", 96)):
        config = bench.make_config("smmnist_big5_ngf96")
        config.model.n_head_channels = nhc
        config.sampling.subsample = sub
        config.device = "cuda:0"
        net = HipScoreNet(config)
        net.load_state_dict(synthetic.random_state_dict(net, seed=123), strict=True)
        x, cond = synthetic.random_inputs(config, 0, B)
        nets[name] = (net, x.cuda(), cond.cuda(), config.data.num_frames)
    legs = [("n_head_channels=-1", 2), ("n_head_channels=-1", 0), ("stock (96-channel heads)", 0)]
    fps = {l: [] for l in legs}
    ran = {}
    for r in range(rounds):
        for l in legs:
            net, x, cond, nfr = nets[l[0]]
            net.set_option("naive_attn", l[1])

            def call(seed):
                return ddpm_sampler(x, net, cond=cond, final_only=True, denoise=True, subsample_steps=sub, clip_before=True, verbose=False, log=False, seed=seed)[0]
            call(999)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(calls):
                call(1000 + i)
            torch.cuda.synchronize()
            fps[l].append(calls * B * nfr / (time.perf_counter() - t0))
            n = _lib.lib.mcvd_model_profile_read(net._model, None, None, None, None, None, 0)
            ks = [_lib.lib.mcvd_model_op_attention_kernel(net._model, i) for i in range(n)]
            ran[l] = sorted(NAMES[k] for k in ks if k >= 0)
            net.set_option("naive_attn", 0)
    base = sum(fps[legs[0]]) / rounds
    for l in legs:
        m = sum(fps[l]) / rounds
        lines.append(f"{l[0]:26s} naive_attn={l[1]}  {m:9.2f} frames/s  [{', '.join(f'{q:.2f}' for q in fps[l])}]  x{m / base:.2f} of the first row   attention ops ran: "
                     f"{ {k: ran[l].count(k) for k in sorted(set(ran[l]))} }")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--naive-limit", type=float, default=2.0, help="seconds the timed one-thread-per-query launches of one shape may take")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--dims", type=int, nargs="*", default=None, help="a subset of the head dims (an A/B of two builds)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_wide_time.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/attn_wide_time.py measures on the GPU"
    assert args.reps >= 20, "median of at least 20"
    lines = [f"# tools/attn_wide_time.py: {torch.cuda.get_device_name(0)}, one process; HIP events per launch"]
    if args.dims:
        DIMS[:] = [d for d in DIMS if d in args.dims]
    per_op(lines, args.reps, args.naive_limit)
    if not args.no_e2e:
        e2e(lines, args.rounds, args.calls)
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(txt)
    print("written:", args.out)


if __name__ == "__main__":
    main()
