"""Time of FidInception on the GPU (profiles/fid_inception_time.txt): per call of 50 images with HIP events, at 64 x 64 and at 299 x 299
input, next to the same net written with torch's own ops on the same GPU (tests/inception_ref.py's restatement in fp32: F.interpolate,
F.conv2d -> MIOpen, F.batch_norm, the pools, torch.cat) -- what a user with the weights but without this package's kernels would run.

    python tools/fid_inception_time.py            # median of 10 calls per path after 2 warm-up calls, the paths interleaved
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/fid_inception_time.py --prof      # 3 calls per shape for the per-kernel table
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mcvd_pytorch_amd as mcvd  # noqa: E402
from tests import inception_ref as ir  # noqa: E402

BATCH = 50
SIZES = (64, 299)


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
    sd = ir.make_state_dict(11)
    det = mcvd.FidInception(device="cuda:0").load_state_dict(sd)
    sdg = {k: v.cuda() for k, v in sd.items()}
    for S in SIZES:
        x = ir.make_images(11, f"time_{S}", (BATCH, 3, S, S)).cuda()
        got = det(x)[0]
        ref = ir.forward(sdg, x, torch.float32)[3]
        dev = ((got - ref).abs().max() / ref.abs().max()).item()
        fns = {"FidInception": lambda: det(x), "torch ops": lambda: ir.forward(sdg, x, torch.float32)}
        if prof:
            for _ in range(3):
                fns["FidInception"]()
            torch.cuda.synchronize()
            print(f"{S} x {S}: 3 calls of FidInception, batch {BATCH}")
            continue
        res = {k: [] for k in fns}
        for k, f in fns.items():
            timed(f, 2)
        for _ in range(5):
            for k, f in fns.items():
                res[k] += timed(f, 2)
        print(f"{BATCH} images of {S} x {S}: max |FidInception - torch ops| / max |torch ops| of the 2048 features {dev:.2e}")
        for k, ts in res.items():
            med = statistics.median(ts)
            print(f"    {k:14s} median {med:9.3f} ms   min {min(ts):9.3f}   max {max(ts):9.3f}   ({len(ts)} calls)   "
                  f"{BATCH / med * 1e3:8.1f} images/s   {5.7 * BATCH / med:6.2f} TFLOP/s at 5.7 GFLOP per image")


if __name__ == "__main__":
    main()
