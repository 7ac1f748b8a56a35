"""GPU: runner.evaluate_video_gen on the HIP path against the REAL `NCSNRunner.video_gen(train=False)` run to its return (fixtures
tests/golden/video_gen_mode_*.pt, tools/gen_video_gen_mode_golden.py; cases and helpers in tests/test_video_gen_mode_cpu.py), the shard
invariance of a seeded evaluation, and load_model_from_ckpt's round trip.

Gates, all taken from the tests of the parts:
  * every sampler call's frames (HipScoreNet + this package's sampler on the recorded block init and step noise): 1e-4, the gate of
    tests/test_gpu_video_tasks.py.  The wrapper then hands the reference's own frames on, so the metrics see exactly what the reference's saw;
  * MSE / PSNR / SSIM keys: tests/test_gpu_video_metrics.py's _mse_gates / _check_summary (3 x the recorded fp32-vs-fp64 distance of the
    per-video MSE, floored at 1 ulp; SSIM 1e-9);
  * embeddings of the stand-in detector on the device: 8 x the fixture's feat_dev (tests/test_gpu_fvd.py); the detector wrapper then
    hands the reference's embeddings on, and the FVD keys are held to that file's relative 1e-7;
  * ckpt, preds_per_test, the key order, the aliases (equal to their sources) and the saved dicts' shapes: exact;
  * shard invariance and the sampler_fn round trip: bit-identical."""
import os

import numpy as np
import pytest
import torch

from oracle import synth
from oracle.gen_runner_golden import runner_config
from tests import fvd_ref
from tests.test_fvd_cpu import RTOL_SINGULAR
from tests.test_gpu_fvd import GATE_FACTOR
from tests.test_gpu_video_metrics import LOG10E10, _check_summary, _mse_gates
from tests.test_video_gen_mode_cpu import (CASES, _write_checkpoint, mode_batches, mode_config, mode_fixture, namespace_to_dict,
                                           replaying_sampler, same_value, step_noise)
from tests.test_video_tasks_cpu import TOL

pytestmark = pytest.mark.gpu


def _hip_net(cfg):
    from mcvd_pytorch_amd.scorenet import HipScoreNet
    cfg.device = "cuda:0"
    net = HipScoreNet(cfg)
    net.load_state_dict(synth.make_state_dict(cfg, seed=123), strict=True)
    return net.eval()


def _replaying_detector(g, det, devs):
    """The stand-in on the device, call by call in the runner's order -- per batch real (1), fake (1), fake (3) --, held to the fixture's
    embeddings; the fixture's rows are handed on."""
    e, ppt = g["embeddings"], g["preds_per_test"]
    order, at = [], {}
    for _ in range(g["max_data_iter"]):
        order += ["real_embeddings", "fake_embeddings"] + (["fake_embeddings3"] if g["gates"][2] else [])
    n = [0]

    def detector(x, **kw):
        assert kw == dict(rescale=False, resize=False, return_features=True) and x.is_cuda and len(x) <= 10
        name = order[n[0]]
        n[0] += 1
        a = at.get(name, 0)
        want = e[name][a:a + len(x)]
        at[name] = a + len(x)
        assert len(want) == len(x) == (g["batch"] // ppt if name.startswith("real") else g["batch"]), (name, len(x))
        devs.append((det(x, **kw).double().cpu() - want).abs().max().item())
        return want.cuda()
    return detector, n, order


@pytest.mark.parametrize("case", CASES)
def test_mode_on_the_hip_path_against_the_real_runner(golden_dir, tmp_path, capsys, case):
    from mcvd_pytorch_amd import evaluate_video_gen
    from mcvd_pytorch_amd.samplers import get_sampler
    g = mode_fixture(golden_dir, case)
    cfg = mode_config(g)
    net = _hip_net(cfg)
    bound = get_sampler(cfg)
    seen, errs, inits, devs, lines = [], [], [0], [], []

    def run_and_replay(call, x, scorenet, cond, kw):
        assert x.is_cuda and cond.is_cuda, "frames left the device between the batch and the sampler"
        assert (cond.cpu() - g["call_cond"][call]).abs().max().item() <= TOL
        out = bound(x, scorenet, cond=cond, noise=step_noise(g, call, tuple(x.shape)).cuda(), **kw)
        errs.append((out[-1].cpu() - g["call_out"][call]).abs().max().item())
        assert errs[-1] <= TOL, f"{case} call {call} ({g['call_phase'][call]} block {g['call_block'][call]}): {errs[-1]:.3e}"
        return g["call_out"][call].cuda().unsqueeze(0)

    def init_noise_fn(block, shape, dev):
        inits[0] += 1
        return g["x_init"][inits[0] - 1].to(dev)
    fvd = None
    if g["fvd"]:
        fvd, n_det, order = _replaying_detector(g, fvd_ref.StandInDetector(g["seed"]).cuda().eval(), devs)
    out = evaluate_video_gen(cfg, net, mode_batches(g), ckpt=0, sampler=replaying_sampler(g, seen, check=run_and_replay),
                             init_noise_fn=init_noise_fn, fvd=fvd, out_dir=str(tmp_path), log=lines.append)
    capsys.readouterr()
    assert len(seen) == len(g["call_phase"]) == inits[0]
    print(f"  {case}: {len(seen)} sampler calls, max frame error {max(errs):.3e} (gate {TOL})")
    files = sorted(os.listdir(tmp_path))
    assert files == g["files"], (files, g["files"])
    for f, shapes in g["saved"].items():
        dd = torch.load(tmp_path / f, weights_only=True)
        assert {k: tuple(v.shape) for k, v in dd.items()} == shapes and all(not v.is_cuda for v in dd.values()), f
    if g["returned"] is None:
        assert out is None and lines == []
        return
    want = g["returned"]
    assert list(out) == [k for k in g["returned_keys"] if "lpips" not in k]
    assert out["ckpt"] == want["ckpt"] == 0 and out["preds_per_test"] == want["preds_per_test"] and type(out["preds_per_test"]) is int
    for ph, key in ((1, ""), (2, "2")):
        if g["vid_mse" + key] is None:
            assert f"mse{key}" not in out
            continue
        ref = g["vid_mse" + key].astype(np.float64)
        gate = _mse_gates(g["vid_mse" + key], g["vid_mse64"][ph])
        _check_summary(out, want, gate.max(), ref.min(), float((LOG10E10 * np.log(1 / ref)).max()), sfx=key)
    fvd_keys = [k for k in g["returned_keys"] if k.startswith("fvd")]
    if g["fvd"]:
        assert n_det[0] == len(order) and fvd_keys
        print(f"  {case}: embeddings max {max(devs):.3e} = {max(devs) / g['feat_dev']:.2f} x feat_dev (gate {GATE_FACTOR})")
        assert max(devs) <= GATE_FACTOR * g["feat_dev"]
        for k in fvd_keys:
            scale = abs(want[k.split("_")[0]]) if ("std" in k or "conf95" in k) else abs(want[k])
            print(f"  {case} {k}: {out[k]!r} against {want[k]!r}: {abs(out[k] - want[k]) / scale:.3e} (gate {RTOL_SINGULAR})")
            assert abs(out[k] - want[k]) <= RTOL_SINGULAR * scale, k
        z = np.load(tmp_path / "video_embeddings_0.npz", allow_pickle=True)
        for k, ref in g["embeddings"].items():
            assert (len(ref) == 0 and len(z[k]) == 0) or np.array_equal(z[k], ref.numpy()), k
    else:
        assert not fvd_keys and not any("fvd" in k for k in out)
    # the aliases: the reference's names, each equal to its source
    first = "interp" if g["overrides"]["data"].get("num_frames_future", 0) else "pred"
    for k in out:
        for prefix, sfx in ((first, ""), ("pred", "2") if g["second_calc"] else (None, None), ("gen", "3")):
            if prefix and k.startswith(prefix + "_"):
                m, _, tail = k[len(prefix) + 1:].partition("_")
                src = m + sfx + ("_" + tail if tail else "")
                if src in out and (prefix != "gen" or m == "fvd"):
                    assert same_value(out[k], out[src]), (k, src)
    assert len(lines) == 2 and lines[1].split(", ", 1)[1].startswith("ckpt:      0, preds_per_test:")


def test_sharded_evaluation_is_the_single_rank_one():
    """Free-running under seed=: 3 clips x preds_per_test 2 whole (6 rows) against the shards of world 2 (2 + 1 clips: 4 + 2 rows), one
    kernel table for the three batch sizes.  The frames of every phase and every value of the merged summary are bit-identical; so are the
    embeddings, in global order."""
    from mcvd_pytorch_amd import VideoMetrics, evaluate_video_gen
    cfg = runner_config("tiny", 6, 8, 10)
    cfg.data.prob_mask_cond, cfg.sampling.fvd, cfg.sampling.preds_per_test, cfg.sampling.max_data_iter = 0.5, True, 2, 1
    net = _hip_net(cfg)
    det = fvd_ref.StandInDetector(11).cuda().eval()
    detector = lambda x, **kw: torch.cat([det(x[i:i + 1], **kw) for i in range(len(x))])      # noqa: E731  (row by row: no batch-size dependence)
    clips = torch.rand(3, 10, 1, 32, 32, generator=torch.Generator().manual_seed(9))
    frames = {}

    def run(shard, tag):
        def sampler(x, scorenet, **kw):
            from mcvd_pytorch_amd.samplers import ddpm_sampler
            kw.update(verbose=False, log=False)                                   # the device loop: quiet
            return ddpm_sampler(x, scorenet, **kw)
        vm = VideoMetrics(cfg, preds_per_test=2, scorenet=net, fvd=detector)
        out = evaluate_video_gen(cfg, net, [clips], ckpt=1, seed=1234, shard=shard, metrics=vm, sampler=sampler, log=lambda ln: None)
        frames[tag] = vm
        return out
    whole = run(None, "whole")
    table = net.get_tuning(6)
    net.set_tuning(4, table)
    net.set_tuning(2, table)
    whole = run(None, "whole")                                                    # again, now that every batch size shares one table
    s0, s1 = run((0, 2), "r0"), run((1, 2), "r1")
    assert s0["shard"] == (0, 2) and [c["rows"] for c in s0["state"]["calls"]] == [4, 4] and [c["rows"] for c in s1["state"]["calls"]] == [2, 2]
    merged = VideoMetrics.merged(cfg, [s0["state"], s1["state"]], scorenet=net)
    ms = merged.summary()
    assert list(ms) == [k for k in whole if k in ms] and {"fvd", "fvd3", "mse", "ssim"} <= set(ms)
    for k, v in ms.items():
        assert same_value(v, whole[k]) and type(v) is type(whole[k]), (k, v, whole[k])
    ew, em = frames["whole"].embeddings(), merged.embeddings()
    for k in ew:
        assert (len(ew[k]) == 0 and len(em[k]) == 0) or np.array_equal(ew[k], em[k]), k
    assert ew["fake_embeddings"].shape[0] == 6 and ew["real_embeddings"].shape[0] == 3 and ew["fake_embeddings3"].shape[0] == 6


def test_sharded_frames_are_bit_identical(tmp_path):
    """The saved dicts of the same runs: rows 0-3 from rank 0 and rows 4-5 from rank 1 are the whole run's rows."""
    from mcvd_pytorch_amd import evaluate_video_gen
    cfg = runner_config("tiny", 6, 4, 10)
    cfg.data.prob_mask_cond, cfg.sampling.preds_per_test, cfg.sampling.max_data_iter = 0.5, 2, 1
    net = _hip_net(cfg)
    clips = torch.rand(3, 6, 1, 32, 32, generator=torch.Generator().manual_seed(10))

    class Quiet:                                                                   # frames only: the metrics are the other test's
        def update(self, *a, **kw):
            pass

        def state(self):
            return {}

        def summary(self):
            return {"preds_per_test": 2}

    def sampler(x, scorenet, **kw):
        from mcvd_pytorch_amd.samplers import ddpm_sampler
        kw.update(verbose=False, log=False)
        return ddpm_sampler(x, scorenet, **kw)
    kw = dict(ckpt=1, seed=77, sampler=sampler, log=lambda ln: None, out_dir=str(tmp_path))
    evaluate_video_gen(cfg, net, [clips], metrics=Quiet(), **kw)
    table = net.get_tuning(6)
    net.set_tuning(4, table)
    net.set_tuning(2, table)
    evaluate_video_gen(cfg, net, [clips], metrics=Quiet(), **kw)
    whole = torch.load(tmp_path / "videos_pred_1.pt", weights_only=True)
    parts = [evaluate_video_gen(cfg, net, [clips], metrics=Quiet(), shard=(r, 2), **kw)["saved"]["videos_pred"] for r in range(2)]
    assert [len(p["pred"]) for p in parts] == [4, 2] and whole["pred"].shape == (6, 4, 32, 32)
    for k in ("cond", "pred", "real"):
        assert torch.equal(torch.cat([p[k] for p in parts]), whole[k]), k
    assert whole["pred"].std() > 0.01 and not torch.equal(whole["pred"][0], whole["pred"][1]), "two predictions of one clip are the same frames"
    # another seed, other frames: the streams are the seed's
    other = evaluate_video_gen(cfg, net, [clips], metrics=Quiet(), shard=(0, 2), **dict(kw, seed=78))["saved"]["videos_pred"]
    assert not torch.equal(other["pred"], parts[0]["pred"]) and torch.equal(other["real"], parts[0]["real"])


def test_init_noise_is_mcvd_randn_at_the_registered_draw_word():
    """The block init z of a seeded run: row b of block i is mcvd_randn's stream (seed + i, offset + b, 2^41) -- keyed by the global row."""
    from mcvd_pytorch_amd.runner import INIT_NOISE_DRAW, _philox_init
    from tests.hiputil import Ctx
    cfg = synth.make_config("tiny")
    net = _hip_net(cfg)
    z = _philox_init(net, 99, 4, (2, 2, 32, 32), net.device)
    torch.cuda.synchronize()
    want = Ctx().randn(6, 2 * 32 * 32, 99, 0, INIT_NOISE_DRAW)
    assert torch.equal(z.reshape(2, -1).cpu(), want[4:6].cpu())
    assert not torch.equal(want[4:6].cpu(), Ctx().randn(2, 2 * 32 * 32, 99, 4, 0).cpu())


def test_load_model_from_ckpt_round_trip(tmp_path):
    """A written checkpoint.pt + config.yml: load_model returns the net with the EMA shadow applied and the parsed config; sampler_fn is
    inverse_data_transform(config, ddpm_sampler(...)[-1].cpu()) bit for bit on the same seed."""
    from mcvd_pytorch_amd import HipScoreNet, ddpm_sampler, inverse_data_transform
    from mcvd_pytorch_amd import load_model_from_ckpt as lm
    cfg0 = runner_config("tiny", 2, 4, 10)
    cfg_dict = namespace_to_dict(cfg0)
    cfg_dict["model"]["ema"] = True
    sd, shadow = _write_checkpoint(str(tmp_path), cfg_dict, ema=True)
    net, config = lm.load_model(str(tmp_path / "checkpoint.pt"), "cuda:0")
    assert isinstance(net, HipScoreNet) and net.device == torch.device("cuda:0") and config.sampling.subsample == 10
    for name, p in net.named_parameters():
        assert torch.equal(p.data.cpu(), shadow[name]), name
    x, cond = synth.make_inputs(config, 2, seed=0)
    fn = lm.get_sampler(config)
    got = fn(x, net, cond, None, seed=5)
    want = inverse_data_transform(config, ddpm_sampler(x.cuda(), net, cond=cond.cuda(), final_only=True, denoise=config.sampling.denoise,
                                                       subsample_steps=10, clip_before=True, seed=5)[-1].to("cpu"))
    assert got.device.type == "cpu" and got.shape == (2, 2, 32, 32) and torch.equal(got, want)
    assert 0.0 <= float(got.min()) and float(got.max()) <= 1.0 and float(got.std()) > 0
    assert not torch.equal(got, fn(x, net, cond, None, seed=6))
