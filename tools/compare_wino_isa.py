"""Compare the generated code of the Winograd kernels between two trees, per kernel symbol (profiles/wino_shared_isa.txt).

    python tools/compare_wino_isa.py OLD_TREE NEW_TREE [--diag]

Compiles conv_wino.cpp, conv_wino2h.cpp, conv_wino3.cpp and conv_wino3p.cpp of both trees to gfx950 assembly with build.py's
flags (--diag: with -DMCVD_DIAG) and reports, for every kernel symbol: the instruction count old -> new, whether every K loop (the
innermost loops that hold MFMAs, delimited as check_wino_isa.py delimits them) is literally the same instruction sequence, and the
kernel descriptor's VGPRs, SGPRs, scratch and LDS ("whole kernel identical": the same instruction sequence from entry to end, block
labels aside).  Exit status 1 when a symbol is missing, a K loop or a descriptor differs, or
an instantiation has more instructions than before.
"""
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_wino_isa import HIPCC, _inner_loop_spans      # noqa: E402

FILES = ("conv_wino", "conv_wino2h", "conv_wino3", "conv_wino3p")
META = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def _instr(lines):
    """instruction lines: labels, directives and comments stripped, block numbers of branch targets normalised"""
    out = []
    for l in lines:
        l = l.split(";")[0].strip()
        if l and not l.startswith(".") and not re.match(r"^\.?\w+:$", l):
            out.append(re.sub(r"\.LBB\d+_\d+", ".LBB", l))
    return out


def kernels(tree, name, diag, td):
    src = os.path.join(tree, "mcvd_pytorch_amd", "csrc", "kernels", name + ".cpp")
    out = os.path.join(td, name + ".s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-I", os.path.join(tree, "include"),
           "-S", "--cuda-device-only", src, "-o", out] + (["-DMCVD_DIAG"] if diag else [])
    subprocess.run(cmd, check=True, capture_output=True)
    text = open(out).read()
    res = {}
    for m in re.finditer(r"^(_ZN4mcvd\w+):[^\n]*\n(.*?)\.Lfunc_end", text, re.S | re.M):
        raw = [l.strip() for l in m.group(2).split("\n") if l.strip()]
        loops = [_instr(raw[lo:hi]) for lo, hi in _inner_loop_spans(raw)]
        res[m.group(1)] = {"n": len(_instr(raw)), "body": _instr(raw), "kloops": [lp for lp in loops if any(i.startswith("v_mfma") for i in lp)]}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M):
        if m.group(1) in res:
            res[m.group(1)]["meta"] = tuple(int(re.search(r"\.amdhsa_" + k + r" (\d+)", m.group(2)).group(1)) for k in META)
    return res


def main():
    old, new = sys.argv[1], sys.argv[2]
    diag = "--diag" in sys.argv[3:]
    bad = 0
    print("symbol  instructions old -> new  K loops  (vgpr, sgpr, scratch, lds)")
    with tempfile.TemporaryDirectory() as t0, tempfile.TemporaryDirectory() as t1, cf.ThreadPoolExecutor(max_workers=8) as ex:
        jobs = {name: (ex.submit(kernels, old, name, diag, t0), ex.submit(kernels, new, name, diag, t1)) for name in FILES}
        for name in FILES:
            a, b = jobs[name][0].result(), jobs[name][1].result()
            for sym in sorted(set(a) | set(b)):
                if sym not in a or sym not in b:
                    print(f"{sym}  ONLY IN {'old' if sym in a else 'new'}")
                    bad += 1
                    continue
                x, y = a[sym], b[sym]
                same_k = x["kloops"] == y["kloops"]
                same_m = x.get("meta") == y.get("meta")
                flag = "" if same_k and same_m and y["n"] <= x["n"] else "  <-- DIFFERS"
                bad += bool(flag)
                print(f"{sym}  {x['n']} -> {y['n']}{' whole kernel identical' if x['body'] == y['body'] else ''}  "
                      f"{len(y['kloops'])} K loop(s) {'identical' if same_k else 'DIFFERENT'}  "
                      f"{x.get('meta')}{'' if same_m else ' -> ' + str(y.get('meta'))}{flag}")
    print("result:", "ok" if not bad else f"{bad} symbol(s) differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
