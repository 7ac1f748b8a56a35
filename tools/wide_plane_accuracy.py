"""Accuracy of the unsplit Winograd kernels (ids 10 / 12 / 4; 24 for the record) on 3x3 layers of more than 1024 input channels on planes of
16 x 16 and larger, next to the direct tile kernel on the same data: profiles/wide_plane_accuracy.txt.

    python tools/wide_plane_accuracy.py [--out profiles/wide_plane_accuracy.txt]

The data, the prologues (raw, affine, affine + SiLU) and the error measures are those of tests/test_gpu_wide_conv.py, whose gate
    err(id) / norm <= max(2 r err(tile) / norm, floor)
tests/test_gpu_wide_plane.py applies with r = the worst err(id) / err(tile) over the NARROW shapes both kernels serve at 16 x 16 --
(Cin, Cout, H) = (672, 288, 16) and (384, 384, 16), B = 2.  This tool prints r per id (the test's R_PLANE) and the same ratio on the test's wide
cases.  Needs a GPU; reads nothing outside the repository.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import test_gpu_wide_conv as T  # noqa: E402
from tests import test_gpu_wide_plane as P  # noqa: E402
from tests.hiputil import Ctx  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_plane_accuracy.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/wide_plane_accuracy.py measures on the GPU"
    ctx = Ctx()
    lines = [f"# tools/wide_plane_accuracy.py: {torch.cuda.get_device_name(0)}; err = max |y - y64| against an fp64 convolution, mag = max conv(|x|, |w|), "
             "scale = max |y64|; tile = conv_shape 2 (direct fp32-MFMA tile kernel) on the same data; prologue 0 raw, 1 affine, 2 affine + SiLU"]
    lines.append("## narrow shapes at 16 x 16 (B = 2): r = the worst err(id) / err(tile) per id")
    r = {}
    for shape in sorted(P.R_PLANE) + [24]:
        for Cin, Cout, H in P.NARROW:
            for case, pro, ran, err, err_tile, mag, scale in T.measure_ratios(ctx, shape, [(2, Cin, 0, Cout, H)]):
                assert ran == shape, (shape, ran)
                r[shape] = max(r.get(shape, 0.0), err / err_tile)
                lines.append(f"id {shape:2d} {case} pro {pro}: err / mag {err / mag:.3e}  tile {err_tile / mag:.3e}  err / scale {err / scale:.3e}  ratio {err / err_tile:.3f}")
                print(lines[-1], flush=True)
    lines.append("R_PLANE = {" + ", ".join(f"{k}: {v:.3f}" for k, v in sorted(r.items()) if k in P.R_PLANE) + "}" +
                 f"   (id 24, one piece, held to its derived bound and not to r: {r[24]:.1f})")
    print(lines[-1], flush=True)
    lines.append("## the wide cases of tests/test_gpu_wide_plane.py")
    worst = {}
    for shape, B, C0, C1, Cout, H in P.CASES:
        for case, pro, ran, err, err_tile, mag, scale in T.measure_ratios(ctx, shape, [(B, C0, C1, Cout, H)]):
            if ran == shape and (shape not in worst or err / err_tile > worst[shape][0]):
                worst[shape] = (err / err_tile, case, pro)
            lines.append(f"id {shape:2d} (ran {ran:2d}) {case} pro {pro}: err / mag {err / mag:.3e}  tile {err_tile / mag:.3e}  err / scale {err / scale:.3e}  "
                         f"ratio {err / err_tile:.3f}" + (f"  (2 r = {2 * r[shape]:.3f})" if shape in P.R_PLANE else "  (one-piece arithmetic: held to its derived bound)"))
            print(lines[-1], flush=True)
    for shape, (ratio, case, pro) in sorted(worst.items()):
        lines.append(f"worst wide ratio, id {shape}: {ratio:.3f} at {case} pro {pro}")
        print(lines[-1], flush=True)
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(txt)
    print("written:", args.out)


if __name__ == "__main__":
    main()
