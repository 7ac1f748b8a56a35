"""GPU: runner.sample on the HIP path against the REAL `NCSNRunner.sample()` (fixtures tests/golden/sample_mode_*.pt,
tools/gen_sample_mode_golden.py; cases and helpers in tests/test_sample_mode_cpu.py).  Every case builds the fixture's checkpoint file from
its seeds and calls mcvd.sample(..., ckpt_dir=) on a HipScoreNet that holds no weights yet, with the recorded z and the step-noise recipe
handed to this package's sampler through `noise=`.

Gates:
  * frames -- every sampler call's output and every returned tensor made of it: 1e-4 absolute, the package's standing sampler-parity
    contract (README; tests/test_gpu_sampler_surface.py).  real / cond / futr / padding take no arithmetic but the transforms': exact;
  * the reference ran on the CPU, where `x_mod.to('cpu')` aliases x_mod and the step noise added in place afterwards shows in its step
    images; a device run appends the copy taken before the noise.  The sampler's step images of `steps` are therefore compared after
    tests/test_oracle_golden.add_back_step_noise, as tests/test_gpu_sampler_surface.py compares them.  The images sample() returns are
    that call's own frames through inverse_data_transform and stretch_image, exactly; the last two, which carry no noise in the
    reference either (the last step adds none, the denoise image is a new tensor), are also held to the reference's at 1e-4;
  * verbose lines: the reference's text and step counters, the three norms to 1e-3 relative (tests/test_gpu_sampler_surface.py);
  * seeded runs, shards, steps_on_device against the default: bit-identical."""
import re

import pytest
import torch

from tests import prdc_ref
from tests.test_oracle_golden import add_back_step_noise
from tests.test_sample_mode_cpu import (check_files, check_plain_result, loaders, recorded_z, replaying_sampler, sample_config,
                                        sample_fixture, write_checkpoint)

pytestmark = pytest.mark.gpu

TOL = 1e-4
LINE = re.compile(r"DDPM: (\d+)/(\d+), grad_norm: ([-0-9.e+]+), image_norm: ([-0-9.e+]+), grad_mean_norm: ([-0-9.e+]+)$")


def _hip_net(cfg):
    from mcvd_pytorch_amd.scorenet import HipScoreNet
    cfg.device = "cuda:0"
    return HipScoreNet(cfg)                               # no weights: sample(ckpt_dir=) loads them


def step_noise(g, call, shape):
    """The step noise of sampler call `call` (the generator's recipe), checked against the recorded sum."""
    z = torch.randn(g["subsample"] - 1, *shape, generator=torch.Generator().manual_seed(g["noise_seed"] + call))
    assert abs(float(z.double().sum()) - g["noise_sums"][call]) <= 1e-6, "torch.randn no longer reproduces the fixture's step noise"
    return z


def run_case(g, cfg, tmp_path, errs, ema_seed="fixture", out_dir=None, log=None, kept=None):
    """mcvd.sample on the HIP net from the fixture's checkpoint file; every sampler call's frames go to `errs` as their distance from
    the reference's (and to `kept` as they are)."""
    from mcvd_pytorch_amd import sample
    from mcvd_pytorch_amd.samplers import get_sampler
    ckpt_dir = tmp_path / f"ckpt_{len(list(tmp_path.iterdir()))}"
    ckpt_dir.mkdir()
    write_checkpoint(ckpt_dir, cfg, g, ema_seed=ema_seed)
    net = _hip_net(cfg)
    bound = get_sampler(cfg)
    seen, n = [], [0]

    def run_on_device(call, x, scorenet, cond, kw):
        assert x.is_cuda and (cond is None or cond.is_cuda), "frames left the device between the batch and the sampler"
        if cond is not None:
            assert torch.equal(cond.cpu(), g["call_cond"][call]), f"call {call}: cond differs from the real runner's"
        noise = step_noise(g, call, tuple(x.shape))
        out = bound(x, scorenet, cond=cond, noise=noise.cuda(), **kw)
        assert out.is_cuda, "the sampler's result left the device"
        if kept is not None:
            kept.append(out.clone())
        got = out.cpu()
        if not kw["final_only"]:
            got = add_back_step_noise(got, "ddpm", dict(subsample_steps=kw["subsample_steps"]), noise, net.alphas.cpu(), net.alphas_prev.cpu(),
                                      net.betas.cpu())
        ref = g["call_out"][call]
        assert got.shape == ref.shape, (got.shape, ref.shape)
        errs.append((got - ref).abs().max().item())
        return out
    batches, cond_batches = loaders(g, cfg)
    kw = {}
    if g["fid"]:
        det = prdc_ref.StandInDetector(5, dims=4, channels=cfg.data.channels * cfg.data.num_frames).cuda().eval()
        kw = dict(real=torch.rand(16, 2, 32, 32, generator=torch.Generator().manual_seed(9)).cuda(), detector=det, cond_batches=cond_batches)
    out = sample(cfg, net, batches, ckpt_dir=str(ckpt_dir), out_dir=out_dir, sampler=replaying_sampler(g, seen, check=run_on_device),
                 init_noise_fn=recorded_z(g, n), log=log, **kw)
    assert len(seen) == g["n_rounds"] == n[0]
    return out, net


def check_lines(mine, ref):
    assert len(mine) == len(ref) == 10
    for a, b in zip(mine, ref):
        ma, mb = LINE.match(a), LINE.match(b)
        assert ma and mb, (a, b)
        assert ma.group(1, 2) == mb.group(1, 2)
        for i in (3, 4, 5):
            va, vb = float(ma.group(i)), float(mb.group(i))
            assert abs(va - vb) <= 1e-3 * abs(vb), (a, b)


@pytest.mark.parametrize("case", ["final", "uncond_init", "future"])
def test_final_only_cases_against_the_real_runner(golden_dir, tmp_path, capsys, case):
    g = sample_fixture(golden_dir, case)
    cfg = sample_config(g)
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    errs = []
    out, net = run_case(g, cfg, tmp_path, errs, out_dir=str(out_dir))
    mine = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("DDPM: ")]
    assert max(errs) <= TOL, f"{case}: sampler frames max error {max(errs):.3e} (gate {TOL})"
    assert out["samples"].is_cuda and out["ckpt"] == g["ckpt"]
    check_plain_result(g, cfg, out, atol=TOL)
    check_files(g, out_dir, out["files"], atol=TOL)
    check_lines(mine, g["call_log_lines"][0])
    if case == "final":
        # the same call on the checkpoint's states[0], the EMA shadow not applied: it must miss the gate, or the EMA load tests nothing
        cfg.model.ema = False
        wrong = []
        run_case(g, cfg, tmp_path, wrong)
        capsys.readouterr()
        print(f"  {case} without the EMA shadow: {max(wrong):.3e}")
        assert max(wrong) > TOL, "the frames do not depend on the EMA shadow"
    print(f"  {case}: sampler frames max error {max(errs):.3e} (gate {TOL})")


def test_steps_case_against_the_real_runner(golden_dir, tmp_path, capsys):
    """final_only=False: 11 step images, on the device; the file names of :1159; and the sampler call repeated with the default
    steps_on_device gives the same values from the CPU."""
    from mcvd_pytorch_amd import inverse_data_transform, stretch_image
    from mcvd_pytorch_amd.samplers import get_sampler
    g = sample_fixture(golden_dir, "steps")
    cfg = sample_config(g)
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    errs, kept = [], []
    out, net = run_case(g, cfg, tmp_path, errs, out_dir=str(out_dir), kept=kept)
    mine = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("DDPM: ")]
    print(f"  steps: sampler step images max error {max(errs):.3e} (gate {TOL})")
    assert max(errs) <= TOL
    assert len(out["steps"]) == 11 and all(t.is_cuda for t in out["steps"]) and out["full_row"].is_cuda
    assert out["files"] == g["files"] == [f"samples_{i:04d}.pt" for i in range(11)] + ["samples_full_7.pt"]
    check_lines(mine, g["call_log_lines"][0])
    frames = kept[0]
    assert tuple(frames.shape) == (11, 3, 1, 32, 32)
    for i in range(11):
        assert torch.equal(out["steps"][i], stretch_image(inverse_data_transform(cfg, frames[i]), 1, 32)), i
        saved = torch.load(str(out_dir / f"samples_{i:04d}.pt"), weights_only=True)
        assert not saved.is_cuda and torch.equal(saved, out["steps"][i].cpu())
    for i in (9, 10):
        assert float((out["steps"][i].cpu() - g["grids"][i]).abs().max()) <= TOL, i
    check_plain_result(dict(g, grids=[t.cpu() for t in out["steps"][:9]] + list(g["grids"][9:])), cfg, out, atol=TOL)
    noise = step_noise(g, 0, tuple(g["x_init"][0].shape))
    # the keyword changes where the images are kept, not their values
    x, cond = g["x_init"][0].cuda(), g["call_cond"][0].cuda()
    kw = dict(cond=cond, final_only=False, denoise=True, subsample_steps=g["subsample"], clip_before=True, noise=noise.cuda())
    bound = get_sampler(cfg)
    on_dev, on_cpu = bound(x, net, steps_on_device=True, **kw), bound(x, net, **kw)
    assert on_dev.is_cuda and on_cpu.device.type == "cpu" and on_dev.shape == on_cpu.shape == (11, 3, 1, 32, 32)
    assert torch.equal(on_dev.cpu(), on_cpu)


@pytest.mark.parametrize("case", ["fid", "fid_init"])
def test_fid_cases_against_the_real_runner(golden_dir, tmp_path, capsys, case):
    """Two rounds on the device; gen_samples against what the reference handed to get_fid_PR; the returned triple is metrics.fid_pr on the
    returned samples with the same stand-in detector."""
    from mcvd_pytorch_amd import metrics
    g = sample_fixture(golden_dir, case)
    cfg = sample_config(g)
    errs, lines = [], []
    out, net = run_case(g, cfg, tmp_path, errs, log=lines.append)
    assert not [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("DDPM: ")], "the FID branch passes verbose=False"
    print(f"  {case}: sampler frames max error {max(errs):.3e} (gate {TOL})")
    assert max(errs) <= TOL
    gen = out["samples"]
    assert gen.is_cuda and tuple(gen.shape) == (6, 2, 32, 32)
    assert float((gen.cpu() - g["gen_samples"]).abs().max()) <= TOL
    det = prdc_ref.StandInDetector(5, dims=4, channels=2).cuda().eval()
    real = torch.rand(16, 2, 32, 32, generator=torch.Generator().manual_seed(9)).cuda()
    fid, precision, recall = metrics.fid_pr(real, gen, det, k=3, scorenet=net)
    assert out["fids"] == {0: fid} and out["precisions"] == {0: precision} and out["recalls"] == {0: recall}
    assert isinstance(fid, float) and fid == fid and 0.0 <= precision <= 1.0 and 0.0 <= recall <= 1.0
    assert lines == ["ckpt: {}, fid: {}, precision: {}, recall: {}".format(0, fid, precision, recall)] and out["files"] == []


def _seeded(g, cfg, tmp_path, sizes):
    """A free-running seeded sample(): whole, whole again, then the two shards of world 2 -- one kernel table for every batch size."""
    from mcvd_pytorch_amd import sample
    ckpt_dir = tmp_path / "ckpt"
    ckpt_dir.mkdir()
    write_checkpoint(ckpt_dir, cfg, g)
    net = _hip_net(cfg)
    kw = {}
    if g["fid"]:
        det = prdc_ref.StandInDetector(5, dims=4, channels=2).cuda().eval()
        kw = dict(real=torch.rand(16, 2, 32, 32, generator=torch.Generator().manual_seed(9)).cuda(), detector=det)

    def run(shard, ckpt=None):
        batches, cond_batches = (None, [g["served"][0]]) if g["fid"] else ([g["served"][0]], None)
        return sample(cfg, net, batches, cond_batches=cond_batches, ckpt_dir=ckpt, seed=4321, shard=shard, log=lambda ln: None, **kw)
    run(None, str(ckpt_dir))
    table = net.get_tuning(sizes[0])
    for b in sizes[1:]:
        net.set_tuning(b, table)
    return run(None), run(None), run((0, 2)), run((1, 2))


def test_seeded_plain_run_is_reproducible_and_shardable(golden_dir, tmp_path, capsys):
    g = sample_fixture(golden_dir, "final")
    cfg = sample_config(g)
    a, b, s0, s1 = _seeded(g, cfg, tmp_path, (4, 2))
    capsys.readouterr()
    assert s0["shard"] == (0, 2) and s1["shard"] == (1, 2) and len(s0["samples"]) == len(s1["samples"]) == 2
    for key in ("samples", "real", "cond", "padding", "full_row"):
        assert torch.equal(a[key], b[key]), key
        assert torch.equal(torch.cat([s0[key], s1[key]]), a[key]), key
    assert a["samples"].std() > 0.01 and not torch.equal(a["samples"][0], a["samples"][1])
    assert (a["nrow"], a["nrow_full"]) == (s0["nrow"], s0["nrow_full"]) == (s1["nrow"], s1["nrow_full"])


def test_seeded_fid_run_is_reproducible_and_shardable(golden_dir, tmp_path):
    """B = 3 over two ranks: 2 + 1 rows of each of the two rounds; the whole run's order is round-major."""
    g = sample_fixture(golden_dir, "fid")
    cfg = sample_config(g)
    a, b, s0, s1 = _seeded(g, cfg, tmp_path, (3, 2, 1))
    assert torch.equal(a["samples"], b["samples"]) and a["fids"] == b["fids"] and a["precisions"] == b["precisions"] and a["recalls"] == b["recalls"]
    assert s0["rounds"] == s1["rounds"] == 2 and "fids" not in s0
    whole = a["samples"].reshape(2, 3, 2, 32, 32)
    parts = torch.cat([s0["samples"].reshape(2, 2, 2, 32, 32), s1["samples"].reshape(2, 1, 2, 32, 32)], dim=1)
    assert torch.equal(parts, whole)
    assert not torch.equal(whole[0], whole[1]), "the two rounds share a noise stream"
