"""Time of the two FVD kernels on the GPU (profiles/fvd_time.txt): fvd_clips (mcvd_fvd_clips) per batch of 10 clips at the shapes of
config 2 and config 5, with the achieved write bandwidth, and feature_stats (mcvd_feature_stats) at FVD and FID size.

    python tools/fvd_time.py            # HIP events per call, median of 20 calls after 3 warm-up calls
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mcvd_pytorch_amd as mcvd  # noqa: E402

# name -> (clips, channels, size, frames per part)
CLIPS = {"config 2 (10 clips, C 1, 64 x 64, 5 cond + 20 pred frames)": (10, 1, 64, (5, 20)),
         "config 5 (10 clips, C 3, 128 x 128, 2 cond + 28 pred frames)": (10, 3, 128, (2, 28))}
STATS = {"FVD size (2 048 rows, d 400)": (2048, 400, 20), "FID size (50 000 rows, d 2 048)": (50000, 2048, 5)}


def timed(fn, n):
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def main():
    g = torch.Generator().manual_seed(1)
    for name, (B, Cc, S, frames) in CLIPS.items():
        parts = [torch.rand(B, t * Cc, S, S, generator=g).cuda() for t in frames]
        f = lambda: mcvd.fvd_clips(parts, Cc)      # noqa: E731
        timed(f, 3)
        ts = timed(f, 20)
        out_bytes = B * 3 * sum(frames) * 224 * 224 * 4
        med = statistics.median(ts)
        print(f"fvd_clips {name}: median {med:8.3f} ms   min {min(ts):8.3f}   max {max(ts):8.3f}   ({len(ts)} calls, torch.empty of the "
              f"output included)   {out_bytes / 1e6:.1f} MB written: {out_bytes / med / 1e6:.0f} GB/s")
    for name, (n, d, reps) in STATS.items():
        x = torch.randn(n, d, generator=g).cuda()
        f = lambda: mcvd.feature_stats(x)          # noqa: E731
        timed(f, 3)
        ts = timed(f, reps)
        med = statistics.median(ts)
        flop = 2.0 * n * d * d            # the full product; the lower triangle of tiles is what is computed
        print(f"feature_stats {name}, fp32 input: median {med:9.3f} ms   min {min(ts):9.3f}   max {max(ts):9.3f}   ({len(ts)} calls)   "
              f"{flop / 1e9:.1f} GFLOP as a full product: {flop / med / 1e9:.2f} TFLOP/s fp64 equivalent")


if __name__ == "__main__":
    main()
