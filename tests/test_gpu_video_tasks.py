"""GPU: MCVD's three video_gen tasks on the HIP path -- HipScoreNet + this package's get_sampler + runner.video_gen(task=...) -- against
the frames and `verbose` lines of the REAL `NCSNRunner.video_gen` (fixtures tests/golden/tiny_runner_task_*.pt, written by
tools/gen_video_tasks_golden.py; cases listed in tests/test_video_tasks_cpu.py), and one interpolation call at the paper's SMMNIST
shape (5 past + 5 future + 5 noisy frames: a 15-channel stem) against the CPU oracle."""
import re

import pytest
import torch

from oracle import synth
from tests.test_video_tasks_cpu import CASES, TOL, check_call_kwargs, task_batch, task_calls, task_config, task_fixture, task_init

pytestmark = pytest.mark.gpu

_LINE = re.compile(r"DDPM: (\d+)/(\d+), grad_norm: ([-0-9.e+]+), image_norm: ([-0-9.e+]+), grad_mean_norm: ([-0-9.e+]+)$")


def _hip_net(cfg):
    from mcvd_pytorch_amd.scorenet import HipScoreNet
    cfg.device = "cuda:0"
    sd = synth.make_state_dict(cfg, seed=123)
    net = HipScoreNet(cfg)
    net.load_state_dict(sd, strict=True)
    return sd, net.eval()


def _assert_same_lines(mine, want):
    """Same text and step counters; the three norms to 1e-3 relative (the rule of the three-edit runner test)."""
    assert len(mine) == len(want) and len(want) > 0, (len(mine), len(want))
    for a, b in zip(mine, want):
        ma, mb = _LINE.match(a), _LINE.match(b)
        assert ma and mb, (a, b)
        assert ma.group(1, 2) == mb.group(1, 2)
        for i in (3, 4, 5):
            va, vb = float(ma.group(i)), float(mb.group(i))
            assert abs(va - vb) <= 1e-3 * abs(vb), (a, b)


@pytest.mark.parametrize("case", CASES)
def test_tasks_on_the_hip_path_against_the_real_runner(golden_dir, capsys, case):
    """Every phase the real runner ran: frames at 1e-4, the sampler kwargs of every block (cond_mask zeros, then ones; it stays out of
    the forward), the `verbose` lines number for number, and case F's RuntimeError before block 1 of (2)."""
    from mcvd_pytorch_amd import runner as r
    from mcvd_pytorch_amd.samplers import ddpm_sampler, get_sampler
    g = task_fixture(golden_dir, case)
    cfg = task_config(g)
    _, net = _hip_net(cfg)
    bound = get_sampler(cfg)
    assert bound.func is ddpm_sampler and bound.keywords == {"config": cfg}
    X = task_batch(cfg, g)
    capsys.readouterr()
    for task, _ in r.video_tasks(cfg):
        _, cond, cond_mask, _ = r.task_conditioning(cfg, X, task)
        idx, seen = task_calls(g, task), []

        def sampler(x, scorenet, cond=None, **kw):
            call = idx[len(seen)]
            seen.append(call)
            check_call_kwargs(g, call, x, cond, kw, cond_tol=TOL)
            return bound(x, scorenet, cond=cond, n_steps_each=0, step_lr=0.0, noise=g["step_noise"][call].cuda(), **kw)
        kw0 = g["call_kwargs"][idx[0]]
        run = lambda: r.video_gen(cfg, net, cond, sampler=sampler, task=task, cond_mask=cond_mask, verbose=kw0["verbose"],  # noqa: E731
                                  log=kw0["log"], init_noise_fn=lambda i, shp, dev: task_init(g, idx, i, shp).to(dev))
        if g["error"] and g["error"]["phase"] == task:
            with pytest.raises(RuntimeError, match=f"left {g['error']['cond_channels']} cond channels"):
                run()
            assert len(seen) == g["error"]["block"] == len(idx)
            continue
        pred = run()
        assert seen == idx and pred.is_cuda
        err = (pred.cpu() - g["pred_raw"][task]).abs().max().item()
        assert err <= TOL, f"{case} {task}: HIP path vs the real runner {err:.3e}"
        mine = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("DDPM: ")]
        _assert_same_lines(mine, [ln for c in idx for ln in g["call_log_lines"][c]])


def test_interp_at_the_paper_shape_on_the_production_kernels():
    """smmnist_big5_ngf96 + num_frames_future = 5 (5 past + 5 future + 5 noisy frames, a 15-channel stem at 64 x 64), one `interp` call,
    DDPM subsample 10, B = 2, on the device loop, against the CPU oracle with the same inits and step noise at 1e-4."""
    from oracle import sampler_ref, unet_ref
    from mcvd_pytorch_amd import runner as r
    from mcvd_pytorch_amd.samplers import get_sampler
    cfg = synth.make_config("smmnist_big5_ngf96")
    cfg.data.num_frames_future = 5
    cfg.sampling.subsample = 10
    d = cfg.data
    B, S, C, nf = 2, d.image_size, d.channels, d.num_frames
    sd, net = _hip_net(cfg)
    assert r.video_tasks(cfg) == [("interp", nf)]
    gen = torch.Generator().manual_seed(11)
    clips = torch.rand(B, d.num_frames_cond + nf + d.num_frames_future, C, S, S, generator=gen)
    real, cond, cond_mask, nfp = r.task_conditioning(cfg, r.data_transform(cfg, clips), "interp")
    assert cond.shape == (B, C * (d.num_frames_cond + d.num_frames_future), S, S) and cond_mask is None and nfp == nf
    z = torch.randn(B, C * nf, S, S, generator=gen)
    noise = torch.randn(cfg.sampling.subsample - 1, B, C * nf, S, S, generator=gen)
    bound, calls = get_sampler(cfg), []

    def sampler(x, scorenet, **kw):
        calls.append(kw)
        return bound(x, scorenet, noise=noise.cuda(), **kw)
    pred = r.video_gen(cfg, net, cond.cuda(), task="interp", cond_mask=cond_mask, sampler=sampler,
                       init_noise_fn=lambda i, shp, dev: z.to(dev)).cpu()
    assert len(calls) == 1 and pred.shape == (B, C * nf, S, S)
    k = [0]

    def fn(i, like):
        k[0] += 1
        return noise[k[0] - 1]
    want = sampler_ref.sample(z.clone(), unet_ref.OracleScoreNet(cfg, sd), cond=cond, kind="ddpm", final_only=True, denoise=True,
                              subsample_steps=10, clip_before=True, noise_fn=fn)[-1]
    assert k[0] == cfg.sampling.subsample - 1
    err = (pred - want).abs().max().item()
    assert err <= 1e-4, f"15-channel-stem interpolation vs the CPU oracle: {err:.3e}"
