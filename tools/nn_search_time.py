"""Time of the nearest-neighbour search on the GPU (profiles/nn_search_time.txt): mcvd_knn_search (kernels/prdc.cpp, fp64, two views, no
n x N matrix) next to the reference's composition with torch's own ops on the same GPU -- torch.cdist twice, torch.min, topk(-d, k)
(evaluation/nearest_neighbor.py:102-109, for all rows at once instead of row by row, everything kept on the device) -- in fp32, as the
reference runs it, and in fp64, the precision of the device path.

    python tools/nn_search_time.py [--out profiles/nn_search_time.txt]      # HIP events per call, median after 3 warm-up calls

FLOP are counted as the two Gram products, 4 d n N, for every variant.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mcvd_pytorch_amd as mcvd  # noqa: E402

# name -> (n queries, N data rows, d, timed calls)
SIZES = {"the reference's own shape (10 x 50 000, d 2 048)": (10, 50000, 2048, 20), "1 000 samples (1 000 x 50 000, d 2 048)": (1000, 50000, 2048, 5)}
K = 10


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


def torch_search(q, q2, r, k=K):
    d = torch.min(torch.cdist(q, r), torch.cdist(q2, r))
    v, i = torch.topk(-d, k=k, dim=1)
    return -v, i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "nn_search_time.txt"))
    args = ap.parse_args()
    lines = [f"knn_search, two views, k = {K}: median of HIP-event times per call after 3 warm-up calls; {torch.cuda.get_device_name(0)}",
             "FLOP: the two Gram products, 4 d n N; the torch rows hold three n x N matrices on the device, the mcvd row none"]
    g = torch.Generator().manual_seed(1)
    for name, (n, N, d, reps) in SIZES.items():
        q, q2, r = (torch.randn(m, d, generator=g).cuda() for m in (n, n, N))
        q64, q264, r64 = q.double(), q2.double(), r.double()
        flop = 4.0 * d * n * N
        variants = (("mcvd knn_search (fp64 MFMA, fp32 input)", lambda: mcvd.knn_search(q, r, K, query2=q2)),
                    ("mcvd knn_search, the data set in 10 pieces", lambda: pieces(q, q2, r)),
                    ("torch cdist x 2 / min / topk, fp32", lambda: torch_search(q, q2, r)),
                    ("torch cdist x 2 / min / topk, fp64", lambda: torch_search(q64, q264, r64)))
        lines.append(f"{name}: {flop / 1e12:.4f} TFLOP")
        want = torch_search(q64, q264, r64)[1]
        for what, fn in variants:
            same = bool((fn()[1] == want).all())
            timed(fn, 3)
            ts = timed(fn, reps)
            med = statistics.median(ts)
            lines.append(f"  {what:46s} median {med:10.3f} ms   min {min(ts):10.3f}   max {max(ts):10.3f}   ({len(ts)} calls)   "
                         f"{flop / med / 1e9:7.2f} TFLOP/s   indices equal to torch fp64: {same}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


def pieces(q, q2, r, parts=10):
    state, step = None, -(-len(r) // parts)
    for at in range(0, len(r), step):
        state = mcvd.knn_search(q, r[at:at + step], K, query2=q2, index_base=at, state=state)
    return state


if __name__ == "__main__":
    main()
