"""Share of sample()'s wall time that is not sampling (profiles/sample_mode_time.txt).

    python tools/sample_mode_time.py [--batch 64] [--repeats 2]

BASELINE config 2 (smmnist_big5_ngf96: 5 past frames, 5 frames per call), DDPM with 100 steps, one batch of B clips, the plain branch of
NCSNRunner.sample() with sampling.final_only true and false (101 step images kept on the device).

Host clock around work that ends in a device synchronise: the whole call, the sampler call inside it (a wrapper that synchronises before
and after) and, beside them, the same sampler call made quietly (verbose = log = False, final_only: the device loop).  sample() always
passes verbose = log = True, so it runs the samplers' host loop with its norm lines.  One untimed call of each first (code objects,
kernel tables, workspaces), then `repeats` timed calls of each, alternating.  Needs the GPU; there is no fallback."""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mcvd_pytorch_amd as mcvd  # noqa: E402
from oracle import synth  # noqa: E402


def sync_clock():
    torch.cuda.synchronize()
    return time.perf_counter()


class Timed:
    """Adds up the synchronised wall time of the calls of a function."""

    def __init__(self, fn):
        self.fn, self.total, self.calls = fn, 0.0, 0

    def __call__(self, *a, **kw):
        t0 = sync_clock()
        out = self.fn(*a, **kw)
        self.total += sync_clock() - t0
        self.calls += 1
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--config", default="smmnist_big5_ngf96")
    ap.add_argument("--subsample", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_mode_time needs the GPU")
    cfg = synth.make_config(args.config)
    cfg.device = "cuda:0"
    d, s = cfg.data, cfg.sampling
    d.dataset = "StochasticMovingMNIST"
    s.subsample, s.batch_size, s.data_init, s.fid, s.inpainting, s.interpolation, s.ckpt_id = args.subsample, args.batch, False, False, False, False, 0
    cfg.model.ema = False
    B, T = args.batch, d.num_frames_cond + d.num_frames
    net = mcvd.HipScoreNet(cfg)
    net.load_state_dict(synth.make_state_dict(cfg, seed=123), strict=True)
    net.eval()
    clips = torch.rand(B, T, d.channels, d.image_size, d.image_size, generator=torch.Generator().manual_seed(1))
    base = mcvd.get_sampler(cfg)
    _, cond, _ = mcvd.conditioning_fn(cfg, mcvd.data_transform(cfg, clips.cuda()), num_frames_pred=d.num_frames)
    z = torch.randn(B, d.channels * d.num_frames, d.image_size, d.image_size, device="cuda")

    def mode(final_only):
        s.final_only = final_only
        sampler = Timed(base)
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = sync_clock()
            out = mcvd.sample(cfg, net, [clips], seed=7, sampler=sampler)
            wall = sync_clock() - t0
        assert sampler.calls == 1 and out["full_row"].is_cuda and (("samples" in out) if final_only else len(out["steps"]) == args.subsample + 1)
        return dict(wall=wall, sampler=sampler.total)

    def quiet():
        t0 = sync_clock()
        base(z, net, cond=cond, final_only=True, denoise=s.denoise, subsample_steps=s.subsample, clip_before=True, verbose=False, log=False, seed=7)
        return dict(wall=sync_clock() - t0, sampler=0.0)

    runs = {"final_only": lambda: mode(True), "all steps": lambda: mode(False), "quiet": quiet}
    for fn in runs.values():
        fn()
    res = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, fn in runs.items():
            res[k].append(fn())
    frames = B * d.num_frames
    q = statistics.median(r["wall"] for r in res["quiet"])
    print(f"{args.config}, B = {B}, DDPM {args.subsample} steps, one sampler call, {frames} frames; median of {args.repeats} calls after one "
          "untimed call (all values in seconds)")
    print(f"  quiet sampler call alone (verbose = log = False, final_only: device loop)   {q:9.3f}   walls {[round(r['wall'], 3) for r in res['quiet']]}")
    for k, name in (("final_only", "sample(), sampling.final_only = True"), ("all steps", f"sample(), sampling.final_only = False ({args.subsample + 1} step images)")):
        wall, smp = (statistics.median(r[key] for r in res[k]) for key in ("wall", "sampler"))
        rest = wall - smp
        print(f"  {name}")
        print(f"    sample() wall {wall:9.3f}   its sampler call {smp:9.3f}   not sampling {rest:8.3f} = {100 * rest / wall:.2f} % of the wall   "
              f"sampler call against the quiet one {100 * (smp / q - 1):+.2f} %   ({frames / wall:.1f} frames/s end to end)")
        print(f"    walls of the calls: {[round(r['wall'], 3) for r in res[k]]}")


if __name__ == "__main__":
    main()
