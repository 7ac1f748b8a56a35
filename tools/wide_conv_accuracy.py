"""Accuracy of the K-split Winograd kernels on 3x3 layers of more than 1024 input channels, next to the direct tile kernel on the same data:
profiles/wide_conv_accuracy.txt.

    python tools/wide_conv_accuracy.py [--out profiles/wide_conv_accuracy.txt]

The data, the prologues (raw, affine, affine + SiLU) and the error measures are those of tests/test_gpu_wide_conv.py, whose gate
    err(id) / mag <= max(2 r err(tile) / mag, floor)
needs r: the worst err(id) / err(tile) over the NARROW shapes both kernels serve -- (Cin, Cout, H) = (672, 288, 16) and (384, 384, 8), B = 2.
This tool prints r per id (the test's R_NARROW) and the same ratio on the test's wide cases.  Needs a GPU; reads nothing outside the repository.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import test_gpu_wide_conv as T  # noqa: E402
from tests.hiputil import Ctx  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_conv_accuracy.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/wide_conv_accuracy.py measures on the GPU"
    ctx = Ctx()
    lines = [f"# tools/wide_conv_accuracy.py: {torch.cuda.get_device_name(0)}; err = max |y - y64| against an fp64 convolution, mag = max conv(|x|, |w|), "
             "scale = max |y64|; tile = conv_shape 2 (direct fp32-MFMA tile kernel) on the same data; prologue 0 raw, 1 affine, 2 affine + SiLU"]
    lines.append("## narrow shapes (B = 2): r = the worst err(id) / err(tile) per id")
    r = {}
    for shape in sorted(T.R_NARROW):
        for Cin, Cout, H in T.NARROW:
            for case, pro, ran, err, err_tile, mag, scale in T.measure_ratios(ctx, shape, [(2, Cin, 0, Cout, H)]):
                if ran != shape:
                    lines.append(f"id {shape:2d} {case}: ran {ran} (the shape does not split that way): not counted")
                    break
                r[shape] = max(r.get(shape, 0.0), err / err_tile)
                lines.append(f"id {shape:2d} {case} pro {pro}: err / mag {err / mag:.3e}  tile {err_tile / mag:.3e}  err / scale {err / scale:.3e}  ratio {err / err_tile:.3f}")
                print(lines[-1], flush=True)
    lines.append("R_NARROW = {" + ", ".join(f"{k}: {v:.3f}" for k, v in sorted(r.items())) + "}")
    print(lines[-1], flush=True)
    lines.append("## the wide cases of tests/test_gpu_wide_conv.py")
    for shape, B, C0, C1, Cout, H in T.CASES:
        for case, pro, ran, err, err_tile, mag, scale in T.measure_ratios(ctx, shape, [(B, C0, C1, Cout, H)]):
            lines.append(f"id {shape:2d} (ran {ran:2d}) {case} pro {pro}: err / mag {err / mag:.3e}  tile {err_tile / mag:.3e}  err / scale {err / scale:.3e}  "
                         f"ratio {err / err_tile:.3f}" + (f"  (2 r = {2 * r[shape]:.3f})" if shape in r else "  (one-piece arithmetic: held to its derived bound)"))
            print(lines[-1], flush=True)
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(txt)
    print("written:", args.out)


if __name__ == "__main__":
    main()
