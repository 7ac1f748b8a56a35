"""CPU: runner.sample -- NCSNRunner.sample() as one call -- against what the REAL `NCSNRunner.sample()` did from its checkpoint file to its
last torch.save (fixtures tests/golden/sample_mode_*.pt, tools/gen_sample_mode_golden.py):

    final         tiny, B = 4         final_only; model.ema with a shadow from a second seed; ckpt_id None -> "latest", checkpoint.pt
    steps         tiny, 1 frame, B = 3   every step image (11 tensors); ckpt_id 7 -> checkpoint_7.pt
    uncond_init   tiny_uncond, B = 3  sampling.data_init on an unconditional net
    future        tiny_spade, B = 2   one cond + one future frame: the futr split, the full row, both nrows
    fid           tiny, 2 rounds of 3    the FID branch; the cond loader holds one batch and starts over
    fid_init      the same from data  cond comes from the init batch

The orchestration runs on a plan-only net (no device): a replaying `sampler=` asserts every call's x_init, cond, cond_mask and kwargs bit
for bit and hands back the recorded output, `init_noise_fn=` the recorded z.  Then stretch_image by hand, the refusals, the shard
bookkeeping and the samplers' `steps_on_device` keyword."""
import argparse
import inspect
import os
from unittest import mock

import pytest
import torch

from oracle import synth
from oracle.gen_runner_golden import runner_config
from tests.golden_io import load_golden

CASES = ["final", "steps", "uncond_init", "future", "fid", "fid_init"]
PLAIN_KW = ("n_steps_each", "step_lr", "verbose", "final_only", "denoise", "subsample_steps", "clip_before", "log", "gamma")
FID_KW = ("n_steps_each", "step_lr", "verbose", "denoise", "subsample_steps", "clip_before", "log", "gamma")      # :1267-1273: no final_only


def sample_fixture(golden_dir, case):
    return load_golden(golden_dir, f"sample_mode_{case}.pt")


def sample_config(g):
    """The config the fixture's run used: oracle/gen_runner_golden.runner_config, the fields NCSNRunner.sample() reads, the case's settings."""
    cfg = runner_config(g["config_name"], g["batch"], 0, g["subsample"])
    s = cfg.sampling
    s.fid, s.inpainting, s.interpolation, s.data_init, s.final_only = False, False, False, False, True
    cfg.fast_fid = argparse.Namespace(pr_nn_k=3)
    for sect in ("data", "model", "sampling"):
        for k, v in g["overrides"][sect].items():
            setattr(getattr(cfg, sect), k, v)
    s.num_frames_pred = cfg.data.num_frames
    return cfg


def write_checkpoint(folder, cfg, g, ema_seed="fixture"):
    """The fixture's checkpoint file from its seeds, in the reference's list format -> (states[0] without prefix, shadow)."""
    ema_seed = g["ema_seed"] if ema_seed == "fixture" else ema_seed
    sd = synth.make_state_dict(cfg, seed=g["sd_seed"])
    shadow = synth.make_state_dict(cfg, seed=ema_seed) if ema_seed is not None else {}
    torch.save([{"module." + k: v for k, v in sd.items()}, {}, 0, 0, shadow], os.path.join(str(folder), g["ckpt_file"]))
    return sd, shadow


class Epochs:
    """The loader of the fixture's run: one batch per pass, pass n yields the n-th batch that was served -- iterating it again is the
    reference's `iter(dataloader)` after StopIteration."""

    def __init__(self, served):
        self.served, self.passes = served, 0

    def __iter__(self):
        n = self.passes
        self.passes += 1
        yield self.served[n], torch.zeros(len(self.served[n]))


def replaying_sampler(g, seen, check=None):
    keys = FID_KW if g["fid"] else PLAIN_KW

    def sampler(x, scorenet, **kw):
        call = len(seen)
        seen.append(call)
        want = g["call_kwargs"][call]
        assert sorted(want) == sorted(keys)
        for k in keys:
            assert kw[k] == want[k] and type(kw[k]) is type(want[k]), (call, k, kw[k], want[k])
        extra = set(kw) - set(keys) - {"seed", "sample_offset"}
        if g["fid"]:                                  # final_only=True is this package's (the reference moves every step to the CPU)
            assert extra == {"cond", "final_only"} and kw["final_only"] is True, sorted(extra)
        else:
            assert extra == {"cond", "cond_mask"} | (set() if want["final_only"] else {"steps_on_device"}), sorted(extra)
            assert g["call_has_cond_mask"][call] and kw.get("steps_on_device", True) is True
            m, wm = kw["cond_mask"], g["call_cond_mask"][call]
            assert (m is None) == (wm is None) and (wm is None or torch.equal(m.cpu().to(wm.dtype), wm)), (call, m, wm)
        assert torch.equal(x.cpu(), g["x_init"][call]), f"call {call}: x_init differs from the real runner's"
        cond = kw["cond"]
        if check is not None:
            return check(call, x, scorenet, cond, {k: v for k, v in kw.items() if k != "cond"})
        if g["call_cond"] is None:
            assert cond is None
        else:
            assert torch.equal(cond, g["call_cond"][call]), f"call {call}: cond differs from the real runner's"
        return g["call_out"][call]
    return sampler


def recorded_z(g, n):
    def init_noise_fn(i, shape, dev):
        assert i == n[0] and tuple(shape) == tuple(g["z"][i].shape)
        n[0] += 1
        return g["z"][i].to(dev)
    return init_noise_fn


def loaders(g, cfg):
    """(batches, cond_batches) as the fixture's run consumed them."""
    if g["served"] is None:
        return None, None
    if g["fid"] and not cfg.sampling.data_init:
        return None, Epochs(g["served"])
    return Epochs(g["served"]), None


def check_plain_result(g, cfg, out, atol=0.0):
    """The returned tensors against what the reference handed to make_grid (and through it to save_image)."""
    d = cfg.data
    S, nf, nc, future = d.image_size, d.num_frames, d.num_frames_cond, getattr(d, "num_frames_future", 0)
    same = (lambda a, b: torch.equal(a.cpu(), b)) if atol == 0.0 else (lambda a, b: a.shape == b.shape and float((a.cpu() - b).abs().max()) <= atol)      # noqa: E731
    grids, nrows = list(g["grids"]), list(g["grid_nrows"])
    if cfg.sampling.final_only:
        assert "steps" not in out and same(out["samples"], grids[0])
        n = 1
    else:
        n = len(out["steps"])
        assert "samples" not in out and n == g["call_out"].shape[1] == 11
        for i in range(n):
            assert same(out["steps"][i], grids[i]), f"step image {i}"
    assert out["nrow"] == nrows[n - 1] and type(out["nrow"]) is int and set(nrows[:n]) == {out["nrow"]}
    if nc == 0:
        assert len(grids) == n and not {"real", "cond", "futr", "full_row", "nrow_full", "padding"} & set(out)
        return
    full = grids[n]
    assert len(grids) == n + 1 and out["nrow_full"] == nrows[n] and type(out["nrow_full"]) is int
    assert same(out["full_row"], full)
    # full = [cond | padding | real | padding | sample (| futr)] along the width
    edges, at = {}, 0
    for name, w in (("cond", nc * S), ("pad0", 2), ("real", nf * S), ("pad1", 2), ("sample", nf * S), ("futr", future * S)):
        edges[name] = (at, at + w)
        at += w
    assert at == full.shape[-1]
    for name in ("cond", "real") + (("futr",) if future else ()):
        assert torch.equal(out[name].cpu(), full[..., edges[name][0]:edges[name][1]]), name
    assert ("futr" in out) == (future > 0)
    assert torch.equal(out["padding"].cpu(), full[..., edges["pad0"][0]:edges["pad0"][1]]) and bool((out["padding"] == 0.5).all())
    assert tuple(out["padding"].shape) == (g["batch"], d.channels, S, 2)


def check_files(g, folder, files, atol=0.0):
    assert files == g["files"] and sorted(os.listdir(str(folder))) == sorted(g["files"])
    for f in files:
        t = torch.load(os.path.join(str(folder), f), weights_only=True)
        assert not t.is_cuda and t.shape == g["saved"][f].shape, f
        assert float((t - g["saved"][f]).abs().max()) <= atol, f


@pytest.mark.parametrize("case", ["final", "steps", "uncond_init", "future"])
def test_plain_branch_matches_the_real_runner(golden_dir, tmp_path, case):
    """The checkpoint that is read and how (EMA or not), the sampler call's x_init, cond, cond_mask and kwargs, every returned tensor, both
    nrows, the label, the written names and their tensors: bit for bit."""
    from mcvd_pytorch_amd import HipScoreNet, sample
    g = sample_fixture(golden_dir, case)
    cfg = sample_config(g)
    ckpt_dir, out_dir = tmp_path / "ckpt", tmp_path / "out"
    ckpt_dir.mkdir(), out_dir.mkdir()
    sd, shadow = write_checkpoint(ckpt_dir, cfg, g)
    net = HipScoreNet(cfg, plan_only=True)
    seen, n = [], [0]
    batches, _ = loaders(g, cfg)
    out = sample(cfg, net, batches, ckpt_dir=str(ckpt_dir), out_dir=str(out_dir), sampler=replaying_sampler(g, seen),
                 init_noise_fn=recorded_z(g, n))
    assert len(seen) == 1 == n[0] and batches.passes == 1
    assert out["ckpt"] == g["ckpt"] and type(out["ckpt"]) is type(g["ckpt"]) and "shard" not in out
    want = shadow if g["ema_seed"] is not None else sd
    for name, p in net.named_parameters():
        assert torch.equal(p.data, want[name]), name
    assert (g["ema_seed"] is not None) == (case == "final") and (case != "final" or not torch.equal(sd[name], shadow[name]))
    check_plain_result(g, cfg, out)
    check_files(g, out_dir, out["files"])


@pytest.mark.parametrize("case", ["fid", "fid_init"])
def test_fid_branch_matches_the_real_runner(golden_dir, tmp_path, case):
    """Two rounds: every sampler call bit for bit, the loader started over, gen_samples as get_fid_PR received them; then what the
    reference never reaches (:1285 raises): the three dicts, the log line of :1286 and samples_{ckpt}.pt of :1301."""
    from mcvd_pytorch_amd import HipScoreNet, sample
    g = sample_fixture(golden_dir, case)
    cfg = sample_config(g)
    ckpt_dir, out_dir = tmp_path / "ckpt", tmp_path / "out"
    ckpt_dir.mkdir(), out_dir.mkdir()
    write_checkpoint(ckpt_dir, cfg, g)
    net = HipScoreNet(cfg, plan_only=True)
    seen, n, lines, scored = [], [0], [], []
    batches, cond_batches = loaders(g, cfg)
    real = torch.zeros(5, 4)

    def fid_pr(real_, fake, detector=None, k=3, batch_size=50, save_feats_path=None, scorenet=None):
        scored.append((real_, fake.clone(), detector, k, save_feats_path, scorenet))
        return g["fid_triple"]
    with mock.patch("mcvd_pytorch_amd.metrics.fid_pr", fid_pr):
        out = sample(cfg, net, batches, cond_batches=cond_batches, ckpt_dir=str(ckpt_dir), real=real, detector="the detector",
                     out_dir=str(out_dir), sampler=replaying_sampler(g, seen), init_noise_fn=recorded_z(g, n), log=lines.append)
    assert len(seen) == g["n_rounds"] == 2 == n[0] and (batches or cond_batches).passes == 2, "the loader was not started over"
    assert g["files"] == [] and g["grids"] == []                                       # the reference stopped at :1285
    gen = g["gen_samples"]
    assert tuple(gen.shape) == (6, 2, 32, 32) and torch.equal(out["samples"], gen)     # [n_rounds B, C nf, S, S]: not (-1, C, S, S)
    assert len(scored) == 1 and scored[0][0] is real and torch.equal(scored[0][1], gen) and scored[0][2] == "the detector"
    assert scored[0][3] == g["pr_nn_k"] == 3 and scored[0][4] is None and scored[0][5] is None
    fid, precision, recall = g["fid_triple"]
    assert out["ckpt"] == g["ckpt"] == 0
    assert out["fids"] == {0: fid} and out["precisions"] == {0: precision} and out["recalls"] == {0: recall}
    assert lines == ["ckpt: {}, fid: {}, precision: {}, recall: {}".format(0, fid, precision, recall)]
    assert out["files"] == ["samples_0.pt"] == os.listdir(str(out_dir))
    assert torch.equal(torch.load(str(out_dir / "samples_0.pt"), weights_only=True), gen)


def test_without_ckpt_dir_the_net_is_used_as_it_is(golden_dir):
    from mcvd_pytorch_amd import HipScoreNet, sample
    g = sample_fixture(golden_dir, "final")
    cfg = sample_config(g)
    net = HipScoreNet(cfg, plan_only=True)
    before = {k: v.data.clone() for k, v in net.named_parameters()}
    out = sample(cfg, net, Epochs(g["served"]), sampler=replaying_sampler(g, []), init_noise_fn=recorded_z(g, [0]))
    assert all(torch.equal(p.data, before[k]) for k, p in net.named_parameters())
    assert out["files"] == [] and torch.equal(out["samples"], g["grids"][0])


def test_stretch_image_by_hand():
    """out[b, c, h, t S + w] = X[b, t ch + c, h, w]: the frames of a row side by side, left to right."""
    from mcvd_pytorch_amd import stretch_image
    B, T, ch, S = 2, 3, 3, 4
    X = torch.arange(B * T * ch * S * S, dtype=torch.float32).reshape(B, T * ch, S, S)
    want = torch.empty(B, ch, S, T * S)
    for b in range(B):
        for t in range(T):
            for c in range(ch):
                for h in range(S):
                    for w in range(S):
                        want[b, c, h, t * S + w] = X[b, t * ch + c, h, w]
    got = stretch_image(X, ch, S)
    assert got.shape == want.shape and torch.equal(got, want)
    assert got.data_ptr() == X.data_ptr() or got.numel() == X.numel()                  # views and one reshape copy: no arithmetic
    assert torch.equal(stretch_image(X[:, :ch], ch, S), X[:, :ch])                     # one frame: unchanged


def _plain_cfg(name="tiny", batch=2, **sampling):
    g = dict(config_name=name, batch=batch, subsample=10, overrides=dict(data={}, model={}, sampling=sampling))
    return sample_config(g)


def _clips(cfg, rows, seed=3):
    d = cfg.data
    T = d.num_frames_cond + d.num_frames + getattr(d, "num_frames_future", 0)
    return torch.rand(rows, T, d.channels, d.image_size, d.image_size, generator=torch.Generator().manual_seed(seed))


def _never(*a, **kw):
    raise AssertionError("the sampler ran")


def test_every_refusal():
    from mcvd_pytorch_amd import HipScoreNet, sample
    cfg = _plain_cfg()
    net = HipScoreNet(cfg, plan_only=True)
    good = [_clips(cfg, 2)]
    for flag in ("inpainting", "interpolation"):                                        # the Langevin samplers of :979 / :1060
        bad = _plain_cfg(**{flag: True})
        with pytest.raises(NotImplementedError, match=flag):
            sample(bad, net, good, sampler=_never)
    bad = _plain_cfg()
    bad.model.version = "SMLD"
    with pytest.raises(NotImplementedError, match="SMLD"):
        sample(bad, net, good, sampler=_never)
    gcfg = _plain_cfg("tiny_gamma", data_init=True)                                    # :1127, :1250
    gnet = HipScoreNet(gcfg, plan_only=True)
    with pytest.raises(NameError, match="used_alphas"):
        sample(gcfg, gnet, good, sampler=_never)
    gcfg.sampling.fid, gcfg.sampling.num_samples4fid = True, 2
    with pytest.raises(NameError, match="used_alphas"):
        sample(gcfg, gnet, good, real=torch.zeros(4, 4), sampler=_never)
    with pytest.raises(ValueError, match="seed"):                                      # torch's generator is not row-keyed
        sample(cfg, net, good, shard=(0, 2), sampler=_never)
    with pytest.raises(ValueError, match="rank, world"):
        sample(cfg, net, good, shard=(2, 2), seed=1, sampler=_never)
    gcfg = _plain_cfg("tiny_gamma")
    with pytest.raises(ValueError, match="init_noise_fn"):
        sample(gcfg, gnet, good, shard=(0, 2), seed=1, sampler=_never)
    with pytest.raises(ValueError, match="batches is needed"):
        sample(cfg, net, None, sampler=_never)
    fcfg = _plain_cfg(fid=True, num_samples4fid=4)
    with pytest.raises(ValueError, match="cond_batches is needed"):
        sample(fcfg, net, None, real=torch.zeros(4, 4), sampler=_never)
    with pytest.raises(ValueError, match="`real` is needed"):
        sample(fcfg, net, None, cond_batches=good, sampler=_never)
    fcfg.sampling.num_samples4fid = 1
    with pytest.raises(ValueError, match="nothing would be sampled"):
        sample(fcfg, net, None, cond_batches=good, real=torch.zeros(4, 4), sampler=_never)


@pytest.mark.parametrize("rows", [1, 3])
def test_a_batch_of_another_length_is_a_value_error(rows):
    """A last batch shorter than sampling.batch_size: the reference's sampler call is mis-shaped (z has batch_size rows); refused before
    any sampler call, in the plain branch and in both loaders of the FID branch."""
    from mcvd_pytorch_amd import HipScoreNet, sample
    cfg = _plain_cfg(batch=2)
    net = HipScoreNet(cfg, plan_only=True)
    z = lambda i, shp, dev: torch.zeros(shp)          # noqa: E731
    with pytest.raises(ValueError, match=f"holds {rows} clips"):
        sample(cfg, net, [_clips(cfg, rows)], sampler=_never, init_noise_fn=z)
    fcfg = _plain_cfg(batch=2, fid=True, num_samples4fid=2)
    with pytest.raises(ValueError, match=f"cond_batches holds {rows} clips"):
        sample(fcfg, net, None, cond_batches=[_clips(cfg, rows)], real=torch.zeros(4, 4), sampler=_never, init_noise_fn=z)
    fcfg.sampling.data_init = True
    with pytest.raises(ValueError, match=f"batches holds {rows} clips"):
        sample(fcfg, net, [(_clips(cfg, rows), None)], real=torch.zeros(4, 4), sampler=_never, init_noise_fn=z)
    with pytest.raises(ValueError, match="batches is empty"):
        sample(cfg, net, [], sampler=_never, init_noise_fn=z)


def row_keyed_sampler(x, scorenet, cond=None, seed=None, sample_offset=0, final_only=True, **kw):
    """Frames that depend on the row's own x and cond, its GLOBAL row index and the call's seed -- what the Philox-keyed samplers guarantee."""
    rows = (sample_offset + torch.arange(len(x), dtype=torch.float32)).view(-1, 1, 1, 1)
    v = torch.tanh(0.1 * x + cond.mean(dim=(1, 2, 3), keepdim=True) + 0.013 * rows + 1e-3 * float(seed % 997) + float(seed >> 20))
    return v.unsqueeze(0) if final_only else torch.stack([v, 0.5 * v])


def row_keyed_z(begin_of):
    def init_noise_fn(i, shape, dev):
        rows = begin_of[0] + torch.arange(shape[0], dtype=torch.float32).view(-1, 1, 1, 1)
        return (rows + i) * torch.ones(shape)
    return init_noise_fn


@pytest.mark.parametrize("world", [2, 3, 5])
@pytest.mark.parametrize("final_only", [True, False])
def test_shards_of_the_plain_branch_concatenate_to_the_whole(world, final_only):
    """B = 4 over 2 (2 + 2), 3 (2 + 1 + 1) and 5 ranks (the last one empty): every returned tensor of a rank is the whole run's rows
    shard_rows(B, rank, world); the samplers get the first row as sample_offset; nrow and nrow_full stay the whole batch's; no file."""
    from mcvd_pytorch_amd import HipScoreNet, sample
    from mcvd_pytorch_amd.dist import shard_rows
    cfg = _plain_cfg(batch=4, final_only=final_only, data_init=True)
    net = HipScoreNet(cfg, plan_only=True)
    clips = [_clips(cfg, 4)]
    whole = sample(cfg, net, clips, sampler=row_keyed_sampler, init_noise_fn=row_keyed_z([0]), seed=5)
    assert "shard" not in whole
    parts = []
    for r in range(world):
        begin, end = shard_rows(4, r, world)
        offsets = []

        def sampler(x, scorenet, **kw):
            offsets.append((kw["seed"], kw["sample_offset"], len(x)))
            return row_keyed_sampler(x, scorenet, **kw)
        with mock.patch("torch.save", _never):
            p = sample(cfg, net, clips, sampler=sampler, init_noise_fn=row_keyed_z([begin]), seed=5, shard=(r, world), out_dir="nowhere")
        assert p["shard"] == (r, world) and p["files"] == [] and offsets == ([(5, begin, end - begin)] if end > begin else [])
        assert p["nrow"] == whole["nrow"] and p["nrow_full"] == whole["nrow_full"]
        parts.append(p)
    for key in ("real", "cond", "padding", "full_row") + (("samples",) if final_only else ()):
        assert torch.equal(torch.cat([p[key] for p in parts]), whole[key]), key
    if not final_only:
        nonempty = [p for p in parts if len(p["real"])]
        assert all(len(p["steps"]) == 2 for p in nonempty)
        for i in range(2):
            assert torch.equal(torch.cat([p["steps"][i] for p in nonempty]), whole["steps"][i])


def test_shards_of_the_fid_branch_concatenate_round_by_round():
    """Round i runs under seed + (i << 20); a rank's 'samples' holds its rows of round 0, then of round 1; nothing is scored."""
    from mcvd_pytorch_amd import HipScoreNet, sample
    from mcvd_pytorch_amd.dist import shard_rows
    cfg = _plain_cfg(batch=3, fid=True, num_samples4fid=7)
    net = HipScoreNet(cfg, plan_only=True)
    cond = [_clips(cfg, 3, seed=4), _clips(cfg, 3, seed=5)]
    seeds = []

    def sampler(x, scorenet, **kw):
        seeds.append(kw["seed"])
        return row_keyed_sampler(x, scorenet, **kw)
    with mock.patch("mcvd_pytorch_amd.metrics.fid_pr", lambda *a, **kw: (1.0, 0.5, 0.5)):
        whole = sample(cfg, net, None, cond_batches=cond, real=torch.zeros(4, 4), sampler=sampler, init_noise_fn=row_keyed_z([0]), seed=9,
                       log=lambda ln: None)
    assert seeds == [9, 9 + (1 << 20)] and whole["samples"].shape[0] == 6
    rounds = whole["samples"].reshape(2, 3, *whole["samples"].shape[1:])
    assert not torch.equal(rounds[0], rounds[1])
    for world in (2, 4):
        got = []
        for r in range(world):
            begin, end = shard_rows(3, r, world)
            with mock.patch("mcvd_pytorch_amd.metrics.fid_pr", _never):
                p = sample(cfg, net, None, cond_batches=cond, sampler=row_keyed_sampler, init_noise_fn=row_keyed_z([begin]), seed=9,
                           shard=(r, world))
            assert p["shard"] == (r, world) and p["rounds"] == 2 and "fids" not in p
            got.append(p["samples"].reshape(2, end - begin, *p["samples"].shape[1:]))
        assert torch.equal(torch.cat(got, dim=1), rounds)


def test_steps_on_device_is_a_keyword_of_every_sampler():
    """Accepted by the three samplers (default False) with either value of final_only: the call gets as far as the device -- which a
    plan-only net does not have -- instead of stopping at the keyword.  That it changes no value is tests/test_gpu_sample_mode.py's."""
    from mcvd_pytorch_amd import HipScoreNet, ddim_sampler, ddpm_sampler, fpndm_sampler
    from mcvd_pytorch_amd import samplers
    assert inspect.signature(samplers._sample).parameters["steps_on_device"].default is False
    assert inspect.signature(fpndm_sampler).parameters["steps_on_device"].default is False
    cfg = _plain_cfg()
    net = HipScoreNet(cfg, plan_only=True)
    x, cond = synth.make_inputs(cfg, 2, seed=0)
    for fn in (ddpm_sampler, ddim_sampler, fpndm_sampler):
        for final_only in (True, False):
            for on_device in (True, False):
                with pytest.raises(RuntimeError, match="plan_only"):
                    fn(x, net, cond=cond, subsample_steps=10, final_only=final_only, steps_on_device=on_device)
