"""Every conv kernel's GroupNorm partials and both reducers against float64, for the record: profiles/gn_partials_accuracy.txt.

    python tools/gn_partials_accuracy.py [--out profiles/gn_partials_accuracy.txt]

Runs the cases of tests/test_gpu_gn_partials.py (the same inputs, through the same helper) and prints per case: the kernel id that ran, np,
the worst coefficient error of gn_finalize over the partials relative to the test's gate (1.0 = the gate), and that error's ratio to the
error of a plain two-pass mean / variance of the same y in float32 on the CPU -- the reference's own fp32 error, not a gate.  Then the
worst line per kernel family, and gn_coef on the outlier data of the test.  Needs a GPU; reads nothing outside the repository.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import gn_ref  # noqa: E402
from tests import test_gpu_gn_partials as T  # noqa: E402
from tests.hiputil import Ctx  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gn_partials_accuracy.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/gn_partials_accuracy.py measures on the GPU"
    ctx = Ctx()
    lines = [f"# tools/gn_partials_accuracy.py: {torch.cuda.get_device_name(0)}; the cases of tests/test_gpu_gn_partials.py",
             "# coef / gate: worst |got - want| / (rtol |want| + atol) of gn_finalize over the partials, modes 0 and 1, want = float64 coefficients of the kernel's own y",
             "# fp32 ref / gate: the same for a plain two-pass float32 mean / variance of y on the CPU (mode 0);  x ref = coef / fp32 ref",
             f"{'case':58s} {'ran':>3s} {'np':>4s} {'sum / gate':>11s} {'M2 err / max':>12s} {'coef / gate':>11s} {'fp32 ref / gate':>15s} {'x ref':>8s}"]
    worst = {}
    for case in T.CASES:
        r = T.measure(ctx, case)
        name = T._case_id(case)
        if r["np"] == 0:
            lines.append(f"{name:58s} {r['ran']:3d} {0:4d}   (emits no partials)")
            continue
        m2 = r["m2_err"] / r["m2_max"] if r["m2_max"] > 0 else 0.0
        xref = r["coef_ratio"] / r["ref32_ratio"] if r["ref32_ratio"] > 0 else float("inf")
        lines.append(f"{name:58s} {r['ran']:3d} {r['np']:4d} {r['sum_ratio']:11.3e} {m2:12.3e} {r['coef_ratio']:11.3e} {r['ref32_ratio']:15.3e} {xref:8.2f}")
        fam = gn_ref.KERNELS[case[0]][0] + ("_ksplit" if gn_ref.KERNELS[case[0]][1] else "")
        if fam not in worst or r["coef_ratio"] > worst[fam][0]:
            worst[fam] = (r["coef_ratio"], lines[-1])
    lines.append("## the worst line per family")
    for fam in sorted(worst):
        lines.append(f"{fam:14s} {worst[fam][1]}")
    lines.append("## gn_coef on one outlier per group (tests/test_gpu_gn_partials.py::test_gn_coef_with_an_outlier): coefficients / gate")
    for gs, HW in ((4, 1024), (3, 4096)):
        for value in (1e3, 3e4):
            for where in (0, 1777):
                x = T.outlier_group(gs, HW, value, where)
                shape = ("outlier", 2, 3 * gs, 0, HW, 3, 1, 1)
                mean, var = gn_ref.group_moments([("tensor", x)], HW, 3)
                want = gn_ref.coefficients(mean, var, T.EPS, 0, 3 * gs)
                got = T._gn_coef(ctx, x, shape, 0, {}).cpu()
                ratio = T._ratio(got, want, 2e-5, gn_ref.gate_atol(mean, var, T.EPS, 0, 3 * gs))
                rel = ((got[..., 0].double() - want[..., 0]).abs() / want[..., 0]).max().item()
                lines.append(f"group {gs} x {HW:4d}  value {value:7g} at element {where:4d}: {ratio:9.3e} x the gate, rstd off by {rel:.3e} relative")
    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(txt)
    print("written:", args.out)


if __name__ == "__main__":
    main()
