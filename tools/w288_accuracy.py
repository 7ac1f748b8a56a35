"""Accuracy of the K-split Winograd kernels of four or more parts on 3x3 layers of 2049 .. 2304 input channels, next to the direct tile kernel on the
same data: profiles/w288_accuracy.txt.

    python tools/w288_accuracy.py [--out profiles/w288_accuracy.txt]

The data, the prologues (raw, affine, affine + SiLU) and the error measures are those of tests/test_gpu_wide_conv.py; the cases are those of
tests/test_gpu_w288.py, whose gate  err(id) / mag <= max(2 r err(tile) / mag, floor)  takes r from tests/test_gpu_wide_conv.py's R_NARROW (measured
on narrow shapes by tools/wide_conv_accuracy.py).  Needs a GPU; reads nothing outside the repository.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import test_gpu_w288 as G  # noqa: E402
from tests import test_gpu_wide_conv as T  # noqa: E402
from tests.hiputil import Ctx  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w288_accuracy.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/w288_accuracy.py measures on the GPU"
    ctx = Ctx()
    lines = [f"# tools/w288_accuracy.py: {torch.cuda.get_device_name(0)}; err = max |y - y64| against an fp64 convolution, mag = max conv(|x|, |w|), "
             "scale = max |y64|; tile = conv_shape 2 (direct fp32-MFMA tile kernel) on the same data; prologue 0 raw, 1 affine, 2 affine + SiLU",
             "## the cases of tests/test_gpu_w288.py: (B, C0, C1, Cout, H)"]
    worst = {}
    for shape, B, C0, C1, Cout, H in G.CASES:
        for case, pro, ran, err, err_tile, mag, scale in T.measure_ratios(ctx, shape, [(B, C0, C1, Cout, H)]):
            r = T.R_NARROW.get(shape)
            worst[shape] = max(worst.get(shape, 0.0), err / err_tile)
            lines.append(f"id {shape:2d} (ran {ran:2d}) {case} pro {pro}: err / mag {err / mag:.3e}  tile {err_tile / mag:.3e}  err / scale {err / scale:.3e}  "
                         f"ratio {err / err_tile:.3f}" + (f"  (2 r = {2 * r:.3f})" if r else "  (one-piece arithmetic: held to its derived bound)"))
            print(lines[-1], flush=True)
    lines.append("worst ratio err(id) / err(tile) per id: {" + ", ".join(f"{k}: {v:.3f}" for k, v in sorted(worst.items())) + "}")
    print(lines[-1], flush=True)
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(txt)
    print("written:", args.out)


if __name__ == "__main__":
    main()
