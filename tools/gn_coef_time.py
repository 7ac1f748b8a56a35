"""mcvd_op_gn_coef alone, HIP events per launch, for an A/B of two builds of the library (the lines of profiles/gn_coef_time.txt, (a)).

    [MCVD_LIB_PATH=<other build>/libmcvd_hip.so] python tools/gn_coef_time.py [--label parent] [--rounds 5] [--reps 200] [--out FILE]

Shapes (B 8, C 96, 64x64) and (B 8, C 2304, 8x8), 32 groups, mode 1, randn input.  Per round: 20 warm-up launches, then `reps` launches each
between two events; the round's figure is the median.  Printed: the median of the rounds and their spread (max - min), per shape.  One
process measures one build; alternate processes of the two builds: --out (default results/gn_coef_time.txt) is appended to.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mcvd_pytorch_amd import _lib  # noqa: E402
from tests.hiputil import Ctx, P  # noqa: E402

SHAPES = [(8, 96, 64), (8, 2304, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this build")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "gn_coef_time.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/gn_coef_time.py measures on the GPU"
    ctx = Ctx()
    lines = []
    for B, Cc, H in SHAPES:
        x = torch.randn(B, Cc, H, H, device="cuda")
        emb = torch.randn(B, 2 * Cc, device="cuda") * 0.3
        coef = torch.empty(B, Cc, 2, device="cuda")

        def launch():
            _lib.check(_lib.lib.mcvd_op_gn_coef(ctx.h, P(x), Cc, None, 0, 32, C.c_float(1e-5), 1, P(emb), None, 2 * Cc, 0, P(coef), B, H * H), "op_gn_coef")
        meds = []
        for _ in range(args.rounds):
            for _ in range(20):
                launch()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
            torch.cuda.synchronize()
            for a, b in ev:
                a.record()
                launch()
                b.record()
            torch.cuda.synchronize()
            meds.append(statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3)
        lines.append(f"{args.label:10s} B{B} C{Cc} {H}x{H}: median {statistics.median(meds):7.2f} us, rounds [{', '.join(f'{m:.2f}' for m in meds)}], "
                     f"spread {max(meds) - min(meds):.2f} us  ({Cc * B * H * H * 4 / statistics.median(meds) * 1e-3:.0f} GB/s read)")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
