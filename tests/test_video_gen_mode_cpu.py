"""CPU: runner.evaluate_video_gen -- NCSNRunner.video_gen's test mode as one call -- against what the REAL `NCSNRunner.video_gen(train=False)`
did from its DataLoader to its return (fixtures tests/golden/video_gen_mode_*.pt, tools/gen_video_gen_mode_golden.py):

    gen      tiny, prob_mask_cond 0.5, preds_per_test 2, 8 frames, max_data_iter 2 of 3 batches of 2 clips      (1) + (3)
    interp   tiny_spade, 1 future frame, prob_mask_future 0.5, 5 frames, preds_per_test 1                       (1) + (2)
    beyond   tiny, num_frames_pred beyond the clip length                                                       the None return

The orchestration runs on a plan-only net (no device): a replaying `sampler=` hands back the fixture's frames, `init_noise_fn=` its block
inits, and a recording `metrics=` keeps what each phase hands to the metric code.  Then the return paths, the alias table, the files, the
sharded state()/merged() of VideoMetrics (world 1, 2, 3 and a gloo world-2 run), the Philox draw word and load_model_from_ckpt."""
import math
import os
import re
import socket
import subprocess
import sys
from unittest import mock

import numpy as np
import pytest
import torch

from oracle import synth
from oracle.gen_runner_golden import runner_config
from tests import philox_ref as pr
from tests.golden_io import load_golden

CASES = ["gen", "interp", "beyond"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW_KEYS = ("final_only", "denoise", "subsample_steps", "clip_before", "t_min", "gamma", "verbose", "log")


def mode_fixture(golden_dir, case):
    return load_golden(golden_dir, f"video_gen_mode_{case}.pt")


def mode_config(g):
    """The config the fixture's run used: oracle/gen_runner_golden.runner_config plus the case's settings."""
    cfg = runner_config(g["config_name"], g["batch"], g["nfp"], g["subsample"])
    for k, v in g["overrides"]["data"].items():
        setattr(cfg.data, k, v)
    cfg.sampling.preds_per_test, cfg.sampling.max_data_iter, cfg.sampling.fvd = g["preds_per_test"], g["max_data_iter"], g["fvd"]
    return cfg


def mode_batches(g, pulled=None):
    """The loader of the fixture's run: the batches it served, then copies of the first up to the loader's length -- the loop must stop
    at max_data_iter, as the reference's does (it fetches one batch more and breaks)."""
    for i in range(g["n_batches"]):
        if pulled is not None:
            pulled.append(i)
        yield g["served"][i if i < len(g["served"]) else 0], torch.zeros(len(g["served"][0]))


def step_noise(g, call, shape):
    """The step noise of sampler call `call` (the generator's recipe), checked against the recorded sum."""
    z = torch.randn(g["subsample"] - 1, *shape, generator=torch.Generator().manual_seed(g["noise_seed"] + call))
    assert abs(float(z.double().sum()) - g["noise_sums"][call]) <= 1e-6, "torch.randn no longer reproduces the fixture's step noise"
    return z


class RecordingMetrics:
    """Stand-in for VideoMetrics: keeps what it is handed."""

    def __init__(self, summary):
        self.calls, self._summary = [], summary

    def update(self, pred01, real01, phase=1, cond01=None):
        self.calls.append((phase, pred01.clone(), real01.clone(), cond01.clone()))

    def update_gen(self, pred_uncond01):
        self.calls.append((3, pred_uncond01.clone(), None, None))

    def summary(self):
        return None if self._summary is None else dict(self._summary)

    def embeddings(self):
        return {k: np.zeros((2, 3)) for k in ("real_embeddings", "fake_embeddings")}


def replaying_sampler(g, seen, check=None):
    def sampler(x, scorenet, cond=None, **kw):
        call = len(seen)
        seen.append(call)
        want = g["call_kwargs"][call]
        for k in KW_KEYS:
            assert kw[k] == want[k], (call, k, kw[k], want[k])
        assert set(kw) - set(KW_KEYS) == {"cond_mask"}, sorted(kw)
        m, wm = kw["cond_mask"], g["call_cond_mask"][call]
        assert (m is None) == (wm is None) and (wm is None or torch.equal(m.cpu().to(wm.dtype), wm)), (call, m, wm)
        assert torch.equal(x.cpu(), g["x_init"][call]), call
        if check is None:
            assert torch.equal(cond, g["call_cond"][call]), f"call {call}: cond differs from the real runner's"
            return g["call_out"][call].unsqueeze(0)
        return check(call, x, scorenet, cond, kw)
    return sampler


def summary_of(g):
    """A summary with the fixture's own keys (without ckpt, time and the aliases) for the recording stand-in to return."""
    r = g["returned"]
    if r is None:
        return None
    out = {}
    for k in g["returned_keys"]:
        if k == "time":
            break
        if k != "ckpt":
            out[k] = r[k]
    return out


def same_value(a, b):
    return (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("case", CASES)
def test_orchestration_matches_the_real_runner(golden_dir, tmp_path, case):
    """Every sampler call's cond, cond_mask, block init and kwargs bit for bit; the tensors handed to update / update_gen exactly; the
    call count, the max_data_iter cut and the phase gates; the returned dict, the log lines, the saved dicts and vid_metrics.yml."""
    from mcvd_pytorch_amd import HipScoreNet, evaluate_video_gen
    g = mode_fixture(golden_dir, case)
    cfg = mode_config(g)
    net = HipScoreNet(cfg, plan_only=True)
    seen, inits, pulled, lines = [], [0], [], []
    rec = RecordingMetrics(summary_of(g))

    def init_noise_fn(block, shape, dev):
        call = inits[0]
        inits[0] += 1
        assert g["call_block"][call] == block and tuple(shape) == tuple(g["x_init"][call].shape)
        return g["x_init"][call].to(dev)
    with mock.patch("builtins.print"):
        out = evaluate_video_gen(cfg, net, mode_batches(g, pulled), ckpt=0, sampler=replaying_sampler(g, seen), init_noise_fn=init_noise_fn,
                                 metrics=rec, out_dir=str(tmp_path), log=lines.append)
    assert len(seen) == len(g["call_phase"]) == inits[0]
    assert pulled == list(range(min(g["n_batches"], g["max_data_iter"] + 1))), "the loop did not stop at max_data_iter"
    # the metric code saw the reference's tensors, phase by phase in its order
    want = []
    for i in range(g["max_data_iter"]):
        want.append((1, g["pred_1"][i], g["real_1"][i], g["cond_1"][i]))
        if g["second_calc"]:
            want.append((2, g["pred_2"][i], g["real_2"][i], g["cond_2"][i]))
        if g["gates"][2]:
            want.append((3, g["pred_3"][i], None, None))
    assert [c[0] for c in rec.calls] == [w[0] for w in want]
    for got, w in zip(rec.calls, want):
        for a, b in zip(got[1:], w[1:]):
            assert (a is None and b is None) or torch.equal(a, b), f"phase {w[0]}: not the tensors the reference's metric code saw"
    # the return
    if g["returned"] is None:
        assert out is None and lines == []                                                   # :2192
    want_keys = g["returned_keys"] if g["returned"] is not None else None
    if want_keys is not None:
        assert list(out) == want_keys, "keys or their order differ from the dict the reference writes"
        for k in want_keys:
            if k != "time":
                assert same_value(out[k], g["returned"][k]), k
        assert re.fullmatch(r"\d+:\d\d:\d\d\.\d{3}", out["time"])
        strip = lambda ln: re.sub(r"\d+:\d\d:\d\d\.\d{3}", "T", ln)       # noqa: E731
        assert [strip(ln) for ln in lines] == [strip(ln) for ln in g["format_p"]]
        import yaml
        mine, ref = yaml.safe_load(open(tmp_path / "vid_metrics.yml")), yaml.safe_load(g["yaml"])
        assert list(mine) == list(ref) == sorted(ref)
        assert all(same_value(mine[k], ref[k]) for k in ref if k != "time")
    # the files: the reference's names and dict shapes (the embeddings file of the stand-in is checked by name only)
    files = sorted(os.listdir(tmp_path))
    assert files == g["files"], (files, g["files"])
    for f, shapes in g["saved"].items():
        dd = torch.load(tmp_path / f, weights_only=True)
        assert {k: tuple(v.shape) for k, v in dd.items()} == shapes, f
        assert all(not v.is_cuda for v in dd.values())


def test_beyond_returns_none_through_the_real_metrics(golden_dir):
    """Phase (1) cannot calculate (:1573-1578): VideoMetrics appends zeros without touching the device and the driver returns None (:2192)."""
    from mcvd_pytorch_amd import HipScoreNet, evaluate_video_gen
    g = mode_fixture(golden_dir, "beyond")
    cfg = mode_config(g)
    assert g["returned"] is None and g["yaml"] is None and g["vid_mse_list"] == [0, 0]
    n = [0]

    def init_noise_fn(block, shape, dev):
        n[0] += 1
        return g["x_init"][n[0] - 1]
    lines = []
    with mock.patch("builtins.print"):
        out = evaluate_video_gen(cfg, HipScoreNet(cfg, plan_only=True), mode_batches(g), ckpt=0, sampler=replaying_sampler(g, []),
                                 init_noise_fn=init_noise_fn, log=lines.append)
    assert out is None and lines == []


def _cfg(**data):
    cfg = runner_config("tiny", 4, 8, 10)
    for k, v in data.items():
        setattr(cfg.data, k, v)
    return cfg


def test_early_returns_and_refusals():
    from mcvd_pytorch_amd import HipScoreNet, evaluate_video_gen
    cfg = _cfg()
    net = HipScoreNet(cfg, plan_only=True)
    cfg.sampling.ssim = False
    assert evaluate_video_gen(cfg, net, iter(())) == {}                                       # :1340-1343
    cfg.sampling.fvd = True
    with pytest.raises(ValueError, match="detector"):                                          # the package loads none
        evaluate_video_gen(cfg, net, iter(()))
    cfg.sampling.fvd, cfg.sampling.ssim = False, True
    with pytest.raises(ValueError, match="seed"):                                              # torch's generator is not row-keyed
        evaluate_video_gen(cfg, net, iter(()), shard=(0, 2))
    with pytest.raises(ValueError, match="rank, world"):
        evaluate_video_gen(cfg, net, iter(()), shard=(2, 2), seed=1)
    cfg.sampling.data_init = True
    with pytest.raises(ValueError, match="data_init_batches"):
        evaluate_video_gen(cfg, net, iter(()))
    cfg.model.gamma = True
    with pytest.raises(NameError, match="used_alphas"):                                        # :1496
        evaluate_video_gen(cfg, net, iter(()), data_init_batches=[])
    cfg.model.gamma, cfg.sampling.data_init = False, False
    cfg.data.num_frames_cond = 0
    with pytest.raises(AssertionError, match="has to be conditional"):                         # :1356
        evaluate_video_gen(cfg, net, iter(()))


def test_train_mode_runs_one_batch_with_one_prediction(golden_dir):
    """train=True (:1345-1348, :2288-2289): max_data_iter = preds_per_test = 1 whatever the config says, quiet sampler calls, and the
    summary without 'time' and aliases."""
    from mcvd_pytorch_amd import HipScoreNet, evaluate_video_gen
    g = mode_fixture(golden_dir, "interp")
    cfg = mode_config(g)
    cfg.sampling.max_data_iter, cfg.sampling.preds_per_test = 5, 3
    kws = []

    def sampler(x, scorenet, cond=None, **kw):
        kws.append(kw)
        return torch.zeros_like(x).unsqueeze(0)
    rec = RecordingMetrics({"preds_per_test": 1, "mse": 0.5})
    out = evaluate_video_gen(cfg, HipScoreNet(cfg, plan_only=True), [g["served"][0]] * 3, ckpt=7, train=True, sampler=sampler, metrics=rec,
                             init_noise_fn=lambda b, s, d: torch.zeros(s), log=lambda ln: None)
    assert out == {"ckpt": 7, "preds_per_test": 1, "mse": 0.5}
    assert [c[0] for c in rec.calls] == [1, 2] and len(rec.calls[0][1]) == len(g["served"][0])
    assert all(kw["verbose"] is False and kw["log"] is False for kw in kws)


BRANCHES = [   # data settings -> (prefix of phase (1), phase (2) as pred_, phase (3) as gen_)
    (dict(), "pred", False, False),
    (dict(num_frames_future=1), "interp", False, False),
    (dict(num_frames_future=1, prob_mask_future=0.5), "interp", True, False),
    (dict(prob_mask_cond=0.5), "pred", False, True),
    (dict(num_frames_future=1, prob_mask_future=0.5, prob_mask_cond=0.5), "interp", True, True),
    (dict(num_frames_future=1, prob_mask_future=0.5, prob_mask_cond=0.5, prob_mask_sync=True), "interp", False, True),
]


@pytest.mark.parametrize("data,first,second,third", BRANCHES)
def test_alias_table(data, first, second, third):
    """The six branches of :2296-2365, written out by hand: which keys are copied under which name."""
    from mcvd_pytorch_amd import video_gen_aliases
    groups = lambda sfx: [f"{m}{sfx}{t}" for m in ("mse", "psnr", "ssim", "lpips") for t in ("", "_std", "_conf95")]     # noqa: E731
    fvds = lambda sfx: [f"fvd{sfx}{t}" for t in ("", "_traj_mean", "_traj_std", "_traj_conf95")]                           # noqa: E731
    base = {"ckpt": 0, "preds_per_test": 1}
    for n, k in enumerate(groups("") + fvds("") + groups("2") + fvds("2") + fvds("3")):
        base[k] = float(n)
    out = video_gen_aliases(_cfg(**data), dict(base))
    want = dict(base)
    for m in ("mse", "psnr", "ssim", "lpips", "fvd"):
        tails = ("", "_traj_mean", "_traj_std", "_traj_conf95") if m == "fvd" else ("", "_std", "_conf95")
        for t in tails:
            want[f"{first}_{m}{t}"] = base[f"{m}{t}"]
            if second:
                want[f"pred_{m}{t}"] = base[f"{m}2{t}"]
    if third:
        for t in ("", "_traj_mean", "_traj_std", "_traj_conf95"):
            want[f"gen_fvd{t}"] = base[f"fvd3{t}"]
    assert out == want
    # absent keys (no LpipsNet, a gate off) are skipped, not raised
    thin = {k: v for k, v in base.items() if "lpips" not in k and "fvd" not in k}
    out = video_gen_aliases(_cfg(**data), dict(thin))
    assert not any("lpips" in k or "fvd" in k for k in out) and f"{first}_mse" in out
    # the mask combination the reference has no branch for adds nothing
    assert video_gen_aliases(_cfg(num_frames_future=1, prob_mask_cond=0.5), dict(base)) == base


def test_alias_order_is_the_references(golden_dir):
    g = mode_fixture(golden_dir, "gen")
    from mcvd_pytorch_amd import video_gen_aliases
    r = {k: g["returned"][k] for k in g["returned_keys"][:g["returned_keys"].index("time") + 1]}
    assert list(video_gen_aliases(mode_config(g), r)) == g["returned_keys"]


def test_yaml_merge_and_format_p(tmp_path):
    """write_to_yaml (:2867-2877): a second write merges into the file's dict and sorts; format_p prints a ckpt that is no int as it is."""
    from mcvd_pytorch_amd.runner import _format_p, write_to_yaml
    import yaml
    p = str(tmp_path / "vid_metrics.yml")
    write_to_yaml(p, {"zeta": 1.5, "ckpt": 10, "mse": 0.25})
    write_to_yaml(p, {"mse": 0.125, "alpha": 2.0})
    got = yaml.safe_load(open(p))
    assert got == {"alpha": 2.0, "ckpt": 10, "mse": 0.125, "zeta": 1.5} and list(got) == sorted(got)
    assert _format_p({"ckpt": 5, "preds_per_test": 2, "mse": 0.123456, "time": "0:00:01.000"}) == \
        "ckpt:      5, preds_per_test:  2, mse:0.1235, time:0:00:01.000"
    assert _format_p({"ckpt": "latest", "mse": 1.0}) == "ckpt:latest, mse:1.0000"


# ---- sharding ---------------------------------------------------------------------------------------------------------------------------

def shard_config():
    cfg = runner_config("tiny", 6, 4, 10)
    cfg.sampling.preds_per_test, cfg.sampling.max_data_iter = 2, 2
    return cfg


def shard_batches():
    """Two batches, of 3 and of 2 clips: world 2 splits 2 + 1 and 1 + 1, world 3 leaves rank 2 an empty shard of the second batch."""
    g = torch.Generator().manual_seed(5)
    return [torch.rand(3, 6, 1, 32, 32, generator=g), torch.rand(2, 6, 1, 32, 32, generator=g)]


def row_keyed_sampler(x, scorenet, cond=None, seed=None, sample_offset=0, **kw):
    """Frames that depend on the row's own cond, its GLOBAL row index and the call's seed -- what the Philox-keyed samplers guarantee."""
    rows = (sample_offset + torch.arange(len(x), dtype=torch.float32)).view(-1, 1, 1, 1)
    v = cond.mean(dim=(1, 2, 3), keepdim=True) + 0.013 * rows + 1e-3 * float(seed % 997)
    return torch.tanh(v + torch.linspace(0, 1, x[0].numel()).view(1, *x.shape[1:])).unsqueeze(0)


def stand_in_frame_metrics(pred01, real01, channels, binary=False, scorenet=None, return_grey=False):
    T = pred01.shape[1] // channels
    p, r = pred01.reshape(len(pred01), T, -1), real01.reshape(len(real01), T, -1)
    return ((p - r) ** 2).mean(-1), (p.double() * r.double()).mean(-1)


def run_shard(shard, metrics=None, out_dir=None):
    from mcvd_pytorch_amd import HipScoreNet, VideoMetrics, evaluate_video_gen
    cfg = shard_config()
    vm = metrics if metrics is not None else VideoMetrics(cfg, preds_per_test=2)
    with mock.patch("mcvd_pytorch_amd.metrics.frame_metrics", stand_in_frame_metrics), mock.patch("builtins.print"):
        out = evaluate_video_gen(cfg, HipScoreNet(cfg, plan_only=True), shard_batches(), ckpt=3, sampler=row_keyed_sampler, seed=11,
                                 shard=shard, metrics=vm, out_dir=out_dir, init_noise_fn=lambda b, s, d: torch.zeros(s),
                                 log=lambda ln: None)
    return out, vm


@pytest.mark.parametrize("world", [1, 2, 3])
def test_state_and_merged_over_uneven_worlds(world):
    """Clips of every batch split over `world` ranks (uneven, and once empty), each rank's state() merged: the lists of the whole run,
    batch-major with the ranks in order, and its summary, exactly."""
    from mcvd_pytorch_amd import VideoMetrics
    whole, vm_whole = run_shard(None)
    assert len(vm_whole.vid[1][0]) == 10 and whole["ckpt"] == 3
    outs = [run_shard((r, world)) for r in range(world)]
    if world > 1:
        assert all(set(o) == {"shard", "state", "saved"} and o["shard"] == (r, world) for r, (o, _) in enumerate(outs))
        assert [sum(c["rows"] for c in o["state"]["calls"]) for o, _ in outs] == ([6, 4] if world == 2 else [4, 4, 2])
    states = [vm.state() for _, vm in outs]
    merged = VideoMetrics.merged(shard_config(), states)
    for ph in (1, 2):
        for which in (0, 1):
            a, b = merged.vid[ph][which], vm_whole.vid[ph][which]
            assert len(a) == len(b) and all(type(x) is type(y) and x == y for x, y in zip(a, b)), (ph, which)
    ms, ws = merged.summary(), vm_whole.summary()
    assert list(ms) == list(ws) and all(same_value(ms[k], ws[k]) for k in ws)
    assert merged.state()["calls"] and sum(c["rows"] for c in merged.state()["calls"]) == 10
    with pytest.raises(ValueError, match="one evaluation"):
        VideoMetrics.merged(shard_config(), states + [dict(states[0], preds_per_test=1)])


def test_merged_keeps_embeddings_in_global_order():
    """The embeddings of state() (fp64 host arrays per call) come back batch-major with the ranks in order; phase (3) keeps its reused reals."""
    from mcvd_pytorch_amd import VideoMetrics
    cfg = runner_config("tiny", 4, 8, 10)
    cfg.data.prob_mask_cond, cfg.sampling.fvd = 0.5, True

    def state(rank):
        calls = []
        for batch in (0, 1):
            for ph in (1, 3):
                e = np.full((1, 4), 100.0 * batch + 10.0 * rank + ph)
                calls.append(dict(phase=ph, rows=2, cannot=False, mse=[np.float32(rank)] * 2 if ph == 1 else None,
                                  ssim=[0.5] * 2 if ph == 1 else None, lpips=None, real=e, fake=np.repeat(e + 0.5, 2, 0)))
        return dict(preds_per_test=2, lpips=False, fvd=True, calls=calls)
    vm = VideoMetrics.merged(cfg, [state(0), state(1)], device="cpu")
    e = vm.embeddings()
    assert e["real_embeddings"][:, 0].tolist() == [1.0, 11.0, 101.0, 111.0] and e["real_embeddings3"][:, 0].tolist() == [3.0, 13.0, 103.0, 113.0]
    assert e["fake_embeddings3"][:, 0].tolist() == [3.5, 3.5, 13.5, 13.5, 103.5, 103.5, 113.5, 113.5] and len(e["real_embeddings2"]) == 0
    assert e["real_embeddings"].dtype == np.float64
    with pytest.raises(RuntimeError, match="merged"):
        vm.fvd(torch.zeros(2, 3, 10, 224, 224))                            # it summarises; it holds no detector to measure with


def test_gloo_world_two_returns_the_single_rank_dict(tmp_path):
    """Two gloo ranks (tests/video_gen_mode_worker_cpu.py): shard taken from torch.distributed, one all_gather_object, both ranks return
    the single-process dict and rank 0 alone writes the files, with the rows of both ranks in the saved dicts."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    single_dir = tmp_path / "single"
    single_dir.mkdir()
    whole, _ = run_shard(None, out_dir=str(single_dir))
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "video_gen_mode_worker_cpu.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    for p in procs:
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, err[-3000:]
    got = [torch.load(tmp_path / f"rank{r}.pt", weights_only=False) for r in range(2)]
    for r in got:
        assert list(r["out"]) == list(whole) and all(same_value(r["out"][k], whole[k]) for k in whole if k != "time")
        assert r["collectives"] == 1
    assert sorted(os.listdir(tmp_path / "out0")) == sorted(os.listdir(single_dir)) == ["vid_metrics.yml", "videos_pred_3.pt"]
    assert os.listdir(tmp_path / "out1") == []
    a, b = torch.load(tmp_path / "out0" / "videos_pred_3.pt"), torch.load(single_dir / "videos_pred_3.pt")
    assert all(torch.equal(a[k], b[k]) for k in b) and len(a["pred"]) == 6


# ---- the Philox draw word -----------------------------------------------------------------------------------------------------------------

def test_init_noise_draw_word_is_a_stream_of_its_own():
    """INIT_NOISE_DRAW against every draw word kernels/philox.h registers, under its counter rule (samples below 2^32): the (c1, c3) pair
    of the counter differs from all of them, with and without the gamma bit, and the header lists the word."""
    from mcvd_pytorch_amd.runner import INIT_NOISE_DRAW, _SEED_SHIFT
    assert INIT_NOISE_DRAW == 1 << 41 and _SEED_SHIFT >= 16
    base = list(range(1001)) + [(1 << 32) + k for k in range(1001)]
    registered = base + [w | (1 << 39) for w in base] + [1 << 40, (1 << 40) | (1 << 39)]
    assert INIT_NOISE_DRAW not in registered
    for sample in (0, 1, (1 << 32) - 1):
        seen = {tuple(int(v) for v in pr.counter(sample, w, 5))[1::2] for w in registered}
        assert len(seen) == len(registered)
        for w in (INIT_NOISE_DRAW, INIT_NOISE_DRAW | (1 << 39)):
            c0, c1, c2, c3 = (int(v) for v in pr.counter(sample, w, 5))
            assert (c0, c2) == (5, sample) and (c1, c3) not in seen, hex(w)
    assert pr.counter(0, INIT_NOISE_DRAW, 0)[3] == 1 << 17
    header = open(os.path.join(ROOT, "mcvd_pytorch_amd", "csrc", "kernels", "philox.h")).read()
    assert "bit 41 set" in header and "INIT_NOISE_DRAW" in header


# ---- load_model_from_ckpt ---------------------------------------------------------------------------------------------------------------

def _write_checkpoint(folder, cfg_dict, ema):
    import yaml
    cfg = synth.make_config("tiny")
    sd = synth.make_state_dict(cfg, seed=123)
    shadow = synth.make_state_dict(cfg, seed=124)
    torch.save([{"module." + k: v for k, v in sd.items()}, {}, 0, 0, shadow], os.path.join(folder, "checkpoint.pt"))
    with open(os.path.join(folder, "config.yml"), "w") as f:
        yaml.dump(cfg_dict, f, default_flow_style=False)
    return sd, shadow


def namespace_to_dict(ns):
    return {k: (namespace_to_dict(v) if hasattr(v, "__dict__") else v) for k, v in vars(ns).items() if k not in ("device", "image_mean")}


def test_load_model_reads_the_config_beside_the_checkpoint(tmp_path):
    from mcvd_pytorch_amd import HipScoreNet
    from mcvd_pytorch_amd import load_model_from_ckpt as lm
    cfg_dict = namespace_to_dict(synth.make_config("tiny"))
    cfg_dict["model"]["ema"] = True
    sd, shadow = _write_checkpoint(str(tmp_path), cfg_dict, ema=True)
    with mock.patch.object(lm, "HipScoreNet", lambda config, device: HipScoreNet(config, plan_only=True)):
        net, config = lm.load_model(str(tmp_path / "checkpoint.pt"), "cuda:0")
        assert config.device == torch.device("cuda:0") and config.data.image_size == 32 and config.model.ema is True
        assert net.training is False
        own = dict(net.named_parameters())
        name = next(iter(own))
        assert torch.equal(own[name].data, shadow[name])                   # the EMA shadow went over states[0]
        cfg_dict["model"]["ema"] = False
        _write_checkpoint(str(tmp_path), cfg_dict, ema=False)
        net, config = lm.load_model(str(tmp_path / "checkpoint.pt"), torch.device("cuda:0"))
        assert torch.equal(dict(net.named_parameters())[name].data, sd[name])
    (tmp_path / "config.yml").write_text("- 1\n- 2\n")
    with pytest.raises(ValueError, match="mapping"):
        lm.load_model(str(tmp_path / "checkpoint.pt"), "cuda:0")


def test_get_sampler_from_config_per_version():
    from mcvd_pytorch_amd import load_model_from_ckpt as lm
    from mcvd_pytorch_amd.samplers import ddim_sampler, ddpm_sampler, fpndm_sampler
    cfg = synth.make_config("tiny")
    for version, fn in (("DDPM", ddpm_sampler), ("DDIM", ddim_sampler), ("FPNDM", fpndm_sampler)):
        cfg.model.version = version
        bound = lm.get_sampler_from_config(cfg)
        assert bound.func is fn and bound.keywords == {"config": cfg}
        assert tuple(lm.init_samples(3, cfg).shape) == (3, cfg.data.channels * cfg.data.num_frames, 32, 32)
    del cfg.model.version
    assert lm.get_sampler_from_config(cfg).func is ddpm_sampler                    # the reference's default (:65)
    cfg.model.version = "SMLD"
    with pytest.raises(NotImplementedError):
        lm.get_sampler_from_config(cfg)
    with pytest.raises(NotImplementedError):
        lm.init_samples(2, cfg)
    cfg.model.version, cfg.model.gamma = "DDPM", True
    with pytest.raises(NameError, match="net"):
        lm.init_samples(2, cfg)
    torch.manual_seed(3)
    a = lm.init_samples(2, synth.make_config("tiny"))
    torch.manual_seed(3)
    assert torch.equal(a, torch.randn(2, 2, 32, 32))


def test_sampler_fn_binds_the_references_keywords():
    """get_sampler (:79-94): the bound keywords, the device moves and inverse_data_transform of the last entry on the CPU."""
    from mcvd_pytorch_amd import load_model_from_ckpt as lm
    from mcvd_pytorch_amd.runner import inverse_data_transform
    cfg = runner_config("tiny", 2, 4, 10)
    cfg.sampling.denoise, cfg.sampling.n_steps_each, cfg.sampling.step_lr = True, 3, 0.5
    seen = {}

    def fake(x, scorenet, **kw):
        seen.update(kw, x=x)
        return torch.stack([x * 0, x * 3.0])
    with mock.patch.object(lm, "ddpm_sampler", fake):
        fn = lm.get_sampler(cfg)
        x, cond = torch.randn(2, 2, 32, 32), torch.randn(2, 2, 32, 32)
        out = fn(x, None, cond, None, subsample=5)
    assert torch.equal(out, inverse_data_transform(cfg, x * 3.0)) and out.device.type == "cpu"
    want = dict(n_steps_each=3, step_lr=0.5, just_beta=False, final_only=True, denoise=True, subsample_steps=5, clip_before=True,
                verbose=False, log=False, gamma=False, cond_mask=None, config=cfg)
    assert {k: seen[k] for k in want} == want and torch.equal(seen["cond"], cond)
