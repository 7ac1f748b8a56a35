"""Time of frame_lpips on the GPU (profiles/lpips_time.txt): per call with HIP events, next to frame_metrics on the same frames and to
steps 4-5 of LPIPS written with torch's own ops on the same GPU (batched F.conv2d / max_pool2d over the resized planes this library
produced -- what a user would otherwise run, with the Pillow resize left out in torch's favour).

    python tools/lpips_time.py            # both shapes, median of 10 calls after 2 warm-up calls, the paths interleaved
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/lpips_time.py --prof      # 3 calls per shape for the per-kernel table
"""
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mcvd_pytorch_amd as mcvd  # noqa: E402
from tests import lpips_ref  # noqa: E402

SHAPES = {"config 2 (B 64, T 5, C 1, 64 x 64)": (64, 5, 1, 64), "config 5 (B 64, T 28, C 3, 128 x 128)": (64, 28, 3, 128)}


def torch_lpips(planes, bb, lins, shift, scale, chunk=64):
    """Steps 4-5 with torch ops, fp32, chunks of 64 frames: planes uint8 [2, N, C, 128, 128] on the GPU -> [N]."""
    out = []
    for i in range(0, planes.shape[1], chunk):
        feats = []
        for which in (0, 1):
            u = planes[which, i:i + chunk]
            if u.shape[1] == 1:
                u = u.expand(-1, 3, -1, -1)
            h = ((u.float().div(255) - 0.5) / 0.5 - shift) / scale
            taps = []
            for (idx, _, _, _, _, stride, pad), pool in zip(lpips_ref.CONVS, lpips_ref.POOL_BEFORE):
                if pool:
                    h = F.max_pool2d(h, 3, 2)
                h = F.relu(F.conv2d(h, bb[f"features.{idx}.weight"], bb[f"features.{idx}.bias"], stride=stride, padding=pad))
                taps.append(h)
            feats.append(taps)
        out.append(lpips_ref.distance(feats[0], feats[1], lins)[0])
    return torch.cat(out)


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
    prof = "--prof" in sys.argv
    bb = lpips_ref.make_backbone(7)
    g = torch.Generator().manual_seed(1)
    lins = [torch.rand(c, generator=g) for c in lpips_ref.CHNS]
    net = mcvd.LpipsNet(device="cuda:0").load_backbone(bb).load_linear({f"lin{k}.model.1.weight": lins[k] for k in range(5)})
    bbg = {k: v.cuda() for k, v in bb.items()}
    ling = [v.cuda() for v in lins]
    shift, scale = torch.tensor([-.030, -.088, -.188]).view(1, 3, 1, 1).cuda(), torch.tensor([.458, .448, .450]).view(1, 3, 1, 1).cuda()
    for name, (B, T, Cc, S) in SHAPES.items():
        real = torch.rand(B, T * Cc, S, S, generator=g)
        pred = (real + 0.2 * torch.randn(B, T * Cc, S, S, generator=g)).clamp(0, 1).cuda()
        real = real.cuda()
        val, _, planes = mcvd.frame_lpips(pred, real, Cc, net, return_taps=True)
        planes = planes.reshape(2, B * T, Cc, 128, 128)
        ref = torch_lpips(planes, bbg, ling, shift, scale)
        dev = ((val.reshape(-1) - ref).abs() / ref).max().item()
        fns = {"frame_lpips": lambda: mcvd.frame_lpips(pred, real, Cc, net),
               "frame_metrics": lambda: mcvd.frame_metrics(pred, real, Cc),
               "torch ops, steps 4-5": lambda: torch_lpips(planes, bbg, ling, shift, scale)}
        if prof:
            for _ in range(3):
                fns["frame_lpips"]()
            torch.cuda.synchronize()
            print(f"{name}: 3 calls of frame_lpips")
            continue
        res = {k: [] for k in fns}
        for k, f in fns.items():
            timed(f, 2)
        for _ in range(5):
            for k, f in fns.items():
                res[k] += timed(f, 2)
        print(f"{name}: {B * T} frames, max relative difference frame_lpips vs torch ops {dev:.2e}")
        for k, ts in res.items():
            print(f"    {k:24s} median {statistics.median(ts):9.3f} ms   min {min(ts):9.3f}   max {max(ts):9.3f}   ({len(ts)} calls)")


if __name__ == "__main__":
    main()
