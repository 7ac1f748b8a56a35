"""Per-batch time of the DSM loss (anneal_dsm_score_estimation) at config 2's shape, B = 64, under the committed kernel table, against the
composition the parent commit offered for the same work: torch.randint, torch.randn_like, the perturbation as torch elementwise ops, the
HipScoreNet forward and the torch reduction and mean.  The two are timed interleaved in one process with HIP events (median of --calls
after warm-up, two rounds: the spread between rounds is the A/B's own noise).  The forward is the same code under both.

    python tools/dsm_loss_time.py [--calls 24] [--rounds 2]                 -> one line per round + a summary
    python tools/dsm_loss_time.py --prof                                    a few calls of config 2 (B = 64) and config 5 (B = 8) for
                                                                            rocprofv3 --kernel-trace --stats (dsm_* kernels)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from oracle import synth  # noqa: E402


def make_net(name, B, table=True):
    from mcvd_pytorch_amd import HipScoreNet
    config = synth.make_config(name)
    config.device = "cuda:0"
    net = HipScoreNet(config)
    net.load_state_dict(synth.make_state_dict(config, seed=123), strict=True)
    path = os.path.join(ROOT, "profiles", f"tune_{name}_B{B}_bf16x3.json")
    if table and os.path.exists(path):
        net.set_tuning(B, json.load(open(path))[str(B)])
    elif not table:
        net.set_option("autotune", 0)
    x, cond = synth.make_inputs(config, B, seed=0)
    return config, net.eval(), x.cuda(), cond.cuda()


@torch.no_grad()
def composed(net, x, cond):
    """The parent commit's best composition of losses/dsm.py:27-52 for a DDPM net."""
    labels = torch.randint(0, len(net.alphas), (x.shape[0],), device=x.device)
    z = torch.randn_like(x)
    a = net.alphas[labels].reshape(x.shape[0], 1, 1, 1)
    px = a.sqrt() * x + (1 - a).sqrt() * z
    eps = net(px, labels, cond=cond)
    return (0.5 * (z - eps).square()).reshape(len(x), -1).sum(dim=-1).mean(dim=0)


def timed(fn, n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return [s.elapsed_time(e) for s, e in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--prof", action="store_true")
    a = ap.parse_args()
    from mcvd_pytorch_amd import anneal_dsm_score_estimation
    if a.prof:
        for name, B, table in (("smmnist_big5_ngf96", 64, True), ("cityscapes_big", 8, False)):
            _, net, x, cond = make_net(name, B, table)
            for _ in range(4):
                anneal_dsm_score_estimation(net, x, cond=cond)
            torch.cuda.synchronize()
            print(f"{name} B={B}: per row {x[0].numel()} elements, done")
        return
    _, net, x, cond = make_net("smmnist_big5_ngf96", 64)
    new = lambda: anneal_dsm_score_estimation(net, x, cond=cond)  # noqa: E731
    old = lambda: composed(net, x, cond)  # noqa: E731
    for _ in range(3):
        new(), old()
    torch.cuda.synchronize()
    meds = {"new": [], "parent": []}
    for r in range(a.rounds):
        t = {"new": [], "parent": []}
        for _ in range(a.calls // 4):                          # interleaved: blocks of 4 calls each, alternating
            t["new"] += timed(new, 4)
            t["parent"] += timed(old, 4)
        for k in t:
            meds[k].append(statistics.median(t[k]))
        print(f"round {r + 1}: new {meds['new'][-1]:.3f} ms, parent composition {meds['parent'][-1]:.3f} ms (median of {len(t['new'])} calls each)")
    mn, mp = statistics.median(meds["new"]), statistics.median(meds["parent"])
    spread = max((max(v) - min(v)) / statistics.median(v) for v in meds.values())
    print(f"summary: new {mn:.3f} ms, parent {mp:.3f} ms, new / parent {mn / mp:.4f}; run-to-run spread of the medians {100 * spread:.2f} %")


if __name__ == "__main__":
    main()
