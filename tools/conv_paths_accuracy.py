"""Every conv kernel on every loader / epilogue path and plane shape against float64, for the record: profiles/conv_paths_accuracy.txt.

    python tools/conv_paths_accuracy.py [--out profiles/conv_paths_accuracy.txt]

Runs the cases of tests/test_gpu_conv_paths.py (the same inputs, through the same measure()) and prints every figure per case: the id that
ran and the one that must, err = max |y - y64| / mag, and each gate's value and limit.  The file written holds, per (id that ran, path),
the worst value / limit of every gate over the cases of that path and the case that set it, then the figures nothing is asserted on (the
two-piece ids on structured data), then the worst line of all.  Needs a GPU; reads nothing outside the repository.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import conv_ref as CR  # noqa: E402
from tests import test_gpu_conv_paths as T  # noqa: E402
from tests.hiputil import Ctx  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_paths_accuracy.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/conv_paths_accuracy.py measures on the GPU"
    ctx = Ctx()
    worst, recorded, failed = {}, [], []
    for part, cases in (("one", T.PART_ONE), ("two", T.PART_TWO)):
        for path, c in cases:
            r = T.measure(ctx, c)
            name = CR.case_id(c)
            gates = "  ".join(f"{n}: {v:.3e} / {lim:.3e}" for n, v, lim, _ in r["gates"])
            print(f"part {part} {path:9s} {name:64s} ran {r['ran']:2d} (must: {r['want']})  err {r['err']:.3e}  {gates}"
                  + (f"  np {r['stats']['np']}" if r["stats"] else "") + ("" if r["repeatable"] else "  NOT REPEATABLE"))
            for n, v in r["recorded"]:
                recorded.append(f"{name:64s} ran {r['ran']:2d}  {n}: {v:.3e}")
            try:
                T.check(c, r)
            except AssertionError as e:
                failed.append(f"{name}: {e}")
            for n, v, lim, _ in r["gates"]:
                ratio = v / lim if lim > 0 else (0.0 if v == 0 else float("inf"))
                key = (r["ran"], part, path, n)
                if key not in worst or ratio > worst[key][0]:
                    worst[key] = (ratio, v, lim, r["err"], name)
    lines = [f"# tools/conv_paths_accuracy.py: {torch.cuda.get_device_name(0)}; the cases of tests/test_gpu_conv_paths.py "
             f"({len(T.PART_ONE)} of part one, {len(T.PART_TWO)} of part two)",
             "# per (id that ran, part, path, gate): the worst value / limit over the cases, the value, the limit, that case's err = max |y - y64| / mag, the case",
             f"{'ran':>3s} {'part':4s} {'path':9s} {'gate':22s} {'/ gate':>9s} {'value':>10s} {'limit':>10s} {'err':>10s}  case"]
    for key in sorted(worst):
        ratio, v, lim, err, name = worst[key]
        lines.append(f"{key[0]:3d} {key[1]:4s} {key[2]:9s} {key[3]:22s} {ratio:9.3f} {v:10.3e} {lim:10.3e} {err:10.3e}  {name}")
    lines.append("## recorded, nothing asserted: the two-piece ids on structured data")
    lines += recorded
    top = max((k for k in worst if worst[k][2] > 0), key=lambda k: worst[k][0])
    lines.append("## the worst line")
    lines.append(f"id {top[0]} part {top[1]} {top[2]} {top[3]}: {worst[top][0]:.3f} x the gate ({worst[top][4]})")
    lines.append(f"## cases that miss a check: {len(failed)}")
    lines += failed
    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(txt)
    print("written:", args.out)


if __name__ == "__main__":
    main()
