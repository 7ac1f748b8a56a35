"""Time of precision_recall on the GPU (profiles/fid_pr_time.txt): mcvd_knn_radii and mcvd_manifold_hits (kernels/prdc.cpp, fp64, no
pairwise matrix) next to the reference's algorithm with torch's own ops on the same GPU -- torch.cdist, kthvalue, <=, any, the three
distance matrices kept on the device (evaluation/fid_PR.py:250-259 without its .cpu() calls) -- in fp32, as the reference runs it, and in
fp64, the precision of the device path.

    python tools/fid_pr_time.py [--out profiles/fid_pr_time.txt]      # HIP events per call, median after 3 warm-up calls

FLOP are counted as the three Gram products, 2 d (Nr^2 + Ng^2 + Ng Nr), for every variant.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mcvd_pytorch_amd as mcvd  # noqa: E402

# name -> (Nr, Ng, d, timed calls)
SIZES = {"the configs' size (1 000 x 1 000, d 2 048)": (1000, 1000, 2048, 20), "FID size (10 000 x 10 000, d 2 048)": (10000, 10000, 2048, 5)}
K = 3


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


def torch_precision_recall(feat_r, feat_g, k=K):
    """calculate_precision_recall_full with the blocks kept on the device."""
    NNk_r = torch.cdist(feat_r, feat_r).kthvalue(k + 1).values
    NNk_g = torch.cdist(feat_g, feat_g).kthvalue(k + 1).values
    dist_g_r = torch.cdist(feat_g, feat_r)
    precision = (dist_g_r <= NNk_r).any(dim=1).float().mean().item()
    recall = (dist_g_r.T <= NNk_g).any(dim=1).float().mean().item()
    return precision, recall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fid_pr_time.txt"))
    args = ap.parse_args()
    lines = [f"precision_recall, k = {K}: median of HIP-event times per call after 3 warm-up calls; {torch.cuda.get_device_name(0)}",
             "FLOP: the three Gram products, 2 d (Nr^2 + Ng^2 + Ng Nr); the torch rows hold three N x N matrices on the device, the mcvd row none"]
    g = torch.Generator().manual_seed(1)
    for name, (Nr, Ng, d, reps) in SIZES.items():
        feat_r = torch.randn(Nr, d, generator=g).abs()
        feat_g = torch.randn(Ng, d, generator=g).abs()
        feat_g[:Ng // 2] = feat_g[:Ng // 2] * 0.8 + 0.35 * (37.0 / d) ** 0.5          # the tests' recipe: half of the generated rows inside
        feat_r, feat_g = feat_r.cuda(), feat_g.cuda()
        r64, g64 = feat_r.double(), feat_g.double()
        flop = 2.0 * d * (Nr * Nr + Ng * Ng + Ng * Nr)
        variants = (("mcvd precision_recall (fp64 MFMA, fp32 input)", lambda: mcvd.precision_recall(feat_r, feat_g, K)),
                    ("torch cdist / kthvalue / <= / any, fp32", lambda: torch_precision_recall(feat_r, feat_g)),
                    ("torch cdist / kthvalue / <= / any, fp64", lambda: torch_precision_recall(r64, g64)))
        lines.append(f"{name}: {flop / 1e12:.3f} TFLOP")
        for what, fn in variants:
            value = fn()
            timed(fn, 3)
            ts = timed(fn, reps)
            med = statistics.median(ts)
            lines.append(f"  {what:48s} median {med:10.3f} ms   min {min(ts):10.3f}   max {max(ts):10.3f}   ({len(ts)} calls)   "
                         f"{flop / med / 1e9:7.2f} TFLOP/s   precision {value[0]:.6f} recall {value[1]:.6f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
