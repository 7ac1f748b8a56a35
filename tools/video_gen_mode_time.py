"""Share of evaluate_video_gen's wall time that is not sampling (profiles/video_gen_mode_time.txt).

    python tools/video_gen_mode_time.py [--batch 64] [--repeats 2]

BASELINE config 2 (smmnist_big5_ngf96: 10 past frames, 5 frames per block, 20 predicted -> 4 blocks), DDPM with 100 steps, one batch of
B clips, preds_per_test 1, all three metric groups: MSE / PSNR / SSIM, LPIPS (an LpipsNet with seeded weights: the time does not depend
on the values) and FVD with tests/fvd_ref.py's stand-in detector (a pooling and two small matrix products -- the caller's I3D costs what it
costs and is not this package's; what is measured here is the clip building, the statistics and the distance around it).

Host clock around work that ends in a device synchronise: the whole call, the sampler calls inside it (a wrapper that synchronises before
and after each), metrics.update and metrics.summary.  One untimed call first (code objects, kernel tables, workspaces), then `repeats`
timed calls of each of two variants, alternating: the mode as it runs (verbose = log = True, as the reference passes them: the samplers'
host loop with its norm lines) and the same with quiet sampler calls (the device loop).  Needs the GPU; there is no fallback."""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mcvd_pytorch_amd as mcvd  # noqa: E402
from oracle import synth  # noqa: E402
from tests import fvd_ref, lpips_ref  # noqa: E402


def sync_clock():
    torch.cuda.synchronize()
    return time.perf_counter()


class Timed:
    """Adds up the synchronised wall time of the calls of a function."""

    def __init__(self, fn):
        self.fn, self.total, self.calls = fn, 0.0, 0

    def __call__(self, *a, **kw):
        t0 = sync_clock()
        out = self.fn(*a, **kw)
        self.total += sync_clock() - t0
        self.calls += 1
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--config", default="smmnist_big5_ngf96")
    ap.add_argument("--subsample", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("video_gen_mode_time needs the GPU")
    cfg = synth.make_config(args.config)
    cfg.device = "cuda:0"
    d, s = cfg.data, cfg.sampling
    d.dataset, d.prob_mask_cond, d.prob_mask_future, d.prob_mask_sync = "StochasticMovingMNIST", 0.0, 0.0, False
    s.subsample, s.ssim, s.fvd, s.preds_per_test, s.max_data_iter, s.batch_size, s.data_init = args.subsample, True, True, 1, 1, args.batch, False
    B, T = args.batch, d.num_frames_cond + s.num_frames_pred
    net = mcvd.HipScoreNet(cfg)
    net.load_state_dict(synth.make_state_dict(cfg, seed=123), strict=True)
    net.eval()
    g = torch.Generator().manual_seed(1)
    clips = torch.rand(B, T, d.channels, d.image_size, d.image_size, generator=g)
    lins = [torch.rand(c, generator=g) for c in lpips_ref.CHNS]
    lp = mcvd.LpipsNet(scorenet=net).load_backbone(lpips_ref.make_backbone(7)).load_linear({f"lin{k}.model.1.weight": lins[k] for k in range(5)})
    det = fvd_ref.StandInDetector(11).cuda().eval()
    base = mcvd.get_sampler(cfg)

    def one(quiet):
        def run(x, scorenet, **kw):
            if quiet:
                kw.update(verbose=False, log=False)
            return base(x, scorenet, **kw)
        sampler = Timed(run)
        vm = mcvd.VideoMetrics(cfg, preds_per_test=1, scorenet=net, lpips=lp, fvd=det)
        vm.update, vm.summary = Timed(vm.update), Timed(vm.summary)
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = sync_clock()
            out = mcvd.evaluate_video_gen(cfg, net, [clips], ckpt=0, seed=7, sampler=sampler, metrics=vm, log=lambda ln: None)
            wall = sync_clock() - t0
        assert out is not None and {"mse", "lpips", "fvd", "pred_fvd"} <= set(out) and sampler.calls == -(-s.num_frames_pred // d.num_frames)
        return dict(wall=wall, sampler=sampler.total, update=vm.update.total, summary=vm.summary.total, calls=sampler.calls)

    one(False)
    one(True)
    res = {False: [], True: []}
    for _ in range(args.repeats):
        for quiet in (False, True):
            res[quiet].append(one(quiet))
    frames = B * s.num_frames_pred
    print(f"{args.config}, B = {B}, DDPM {args.subsample} steps, {res[False][0]['calls']} blocks, {frames} predicted frames, one batch; "
          f"median of {args.repeats} calls after one untimed call (all values in seconds)")
    for quiet, name in ((False, "as the mode runs (verbose = log = True: host loop)"), (True, "quiet sampler calls (device loop)")):
        med = {k: statistics.median(r[k] for r in res[quiet]) for k in ("wall", "sampler", "update", "summary")}
        rest = med["wall"] - med["sampler"]
        other = rest - med["update"] - med["summary"]
        print(f"  {name}")
        print(f"    evaluate_video_gen wall {med['wall']:9.3f}   its sampler calls {med['sampler']:9.3f}   not sampling {rest:8.3f} = "
              f"{100 * rest / med['wall']:.2f} % of the wall   ({frames / med['wall']:.1f} frames/s end to end)")
        print(f"    not sampling: metrics.update {med['update']:.3f} (frame metrics, LPIPS, FVD clips + stand-in detector), "
              f"metrics.summary {med['summary']:.3f} (FVD statistics, eigenvalues on the host), the driver's own {other:.3f}")
        print(f"    walls of the calls: {[round(r['wall'], 3) for r in res[quiet]]}")


if __name__ == "__main__":
    main()
