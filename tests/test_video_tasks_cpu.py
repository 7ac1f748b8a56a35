"""CPU: MCVD's three video_gen tasks -- runner.video_tasks, runner.task_conditioning and runner.video_gen(task=...) -- against what the
REAL `NCSNRunner.video_gen` did on the same clips (tools/gen_video_tasks_golden.py drove runners/ncsn_runner.py:1304-1916 through
(1) prediction / interpolation, (2) prediction with the future block masked, (3) unconditional generation, and recorded every
sampler call).

    A  tiny + 1 future frame                          (1) interp, one block
    B  tiny_spade, prob_mask_future 0.5, 5 frames      (1) interp + (2) three blocks, zero future block kept, SPADE cond
    C  tiny cond_emb, prob_mask_cond 0.5, 8 frames,    (1) pred, 4 blocks + (3) gen, 10 frames, 5 blocks
       preds_per_test 2
    D  tiny + future 1, both masks 0.5                 (1) + (2) + (3), (3) with the future block
    E  D with prob_mask_sync                           (1) + (3)
    F  B with one_frame_at_a_time                      (1) as two one-frame blocks; (2) fails at its second block
"""
import pytest
import torch

from oracle import synth
from tests.golden_io import load_golden

CASES = ["A", "B", "C", "D", "E", "F"]
TOL = 1e-4          # the gate of tests/test_runner_cpu.py for DDPM chains on [-1, 1] frames


def task_fixture(golden_dir, case):
    return load_golden(golden_dir, f"tiny_runner_task_{case}.pt")


def task_config(g):
    cfg = synth.make_config(g["config_name"])
    cfg.sampling.num_frames_pred, cfg.sampling.subsample = g["nfp"], g["subsample"]
    for sect, kv in g["overrides"].items():
        for k, v in kv.items():
            setattr(getattr(cfg, sect), k, v)
    return cfg


def task_batch(cfg, g):
    """The rows the shuffling DataLoader served (repeat_interleave'd under preds_per_test), after data_transform."""
    from mcvd_pytorch_amd import runner as r
    return r.data_transform(cfg, g["clips"][g["order"]])


def task_calls(g, task):
    """Indices of the recorded sampler calls of one phase, in block order."""
    idx = [i for i, p in enumerate(g["call_phase"]) if p == task]
    assert [g["call_block"][i] for i in idx] == list(range(len(idx)))
    return idx


def task_init(g, idx, i, shape):
    """The real runner's block-i init of a phase; zeros for case F's block that never samples (the fixture keeps the calls that ran)."""
    return g["x_init"][idx[i]] if i < len(idx) else torch.zeros(shape)


def check_call_kwargs(g, call, x, cond, kw, cond_tol):
    """What the library's block loop hands the sampler against what the real runner handed it on the same call."""
    want = g["call_kwargs"][call]
    for k in ("final_only", "denoise", "subsample_steps", "clip_before", "t_min", "gamma", "verbose", "log"):
        assert kw[k] == want[k], (k, kw[k], want[k])
    m, wm = kw["cond_mask"], g["call_cond_mask"][call]
    assert (m is None) == (wm is None), (m, wm)
    if wm is not None:                                           # gen: zeros at block 0, ones afterwards (:1885-1886)
        assert torch.equal(m.cpu().to(torch.int32), wm)
    assert torch.equal(x.cpu(), g["x_init"][call])
    assert cond.shape == g["call_cond"][call].shape
    assert (cond.cpu() - g["call_cond"][call]).abs().max().item() <= cond_tol


def test_video_tasks_over_the_six_mask_combinations(golden_dir):
    """(1) alone, (1)+(2), (1)+(3), (1)+(2)+(3), (1)+(3) under prob_mask_sync: the phases the real runner ran, in its order, with their
    frame counts; prediction alone from the round-6 runner fixture."""
    from mcvd_pytorch_amd import video_tasks
    for case in CASES:
        g = task_fixture(golden_dir, case)
        cfg = task_config(g)
        assert video_tasks(cfg) == [tuple(p) for p in g["phases"]], case
        ran = list(dict.fromkeys(g["call_phase"] + ([g["error"]["phase"]] if g["error"] else [])))
        assert [t for t, _ in video_tasks(cfg)] == ran, case
    g = load_golden(golden_dir, "tiny_runner_videogen.pt")
    cfg = synth.make_config(g["config_name"])
    cfg.sampling.num_frames_pred = g["nfp"]
    assert video_tasks(cfg) == [("pred", g["nfp"])]
    # (3) is gated on prob_mask_cond alone: the reference's >= 10-frame rule belongs to FVD
    cfg.data.prob_mask_cond = 0.5
    assert video_tasks(cfg) == [("pred", g["nfp"]), ("gen", cfg.data.num_frames_cond + g["nfp"])]


@pytest.mark.parametrize("case", CASES)
def test_task_conditioning_is_the_real_runners(golden_dir, case):
    """real / cond / cond_mask of every conditioning_fn call the real runner made, bit for bit."""
    from mcvd_pytorch_amd import task_conditioning
    g = task_fixture(golden_dir, case)
    cfg = task_config(g)
    X = task_batch(cfg, g)
    assert len(g["cf"]) == len(g["phases"])
    for rec in g["cf"]:
        real, cond, cond_mask, nfp = task_conditioning(cfg, X, rec["phase"])
        w_real, w_cond, w_mask = rec["out"]
        assert nfp == rec["num_frames_pred"]
        assert torch.equal(real, w_real) and torch.equal(cond, w_cond), rec["phase"]
        assert (cond_mask is None) == (w_mask is None) and (w_mask is None or torch.equal(cond_mask, w_mask)), rec["phase"]


def _oracle_sampler(g, idx, net, seen):
    from oracle import sampler_ref

    def sampler(x, scorenet, cond=None, **kw):
        call = idx[len(seen)]
        seen.append(call)
        check_call_kwargs(g, call, x, cond, kw, cond_tol=TOL)
        k = [0]

        def fn(i, like):
            k[0] += 1
            return g["step_noise"][call, k[0] - 1]
        return sampler_ref.sample(x, net, cond=cond, kind="ddpm", final_only=True, denoise=kw["denoise"],
                                  subsample_steps=kw["subsample_steps"], clip_before=kw["clip_before"], t_min=kw["t_min"], noise_fn=fn)
    return sampler


@pytest.mark.parametrize("case", CASES)
def test_task_block_loop_matches_the_real_runner(golden_dir, case):
    """video_gen(task=...) around the CPU oracle net and sampler, fed the real runner's block inits and step noise: the frames of every
    phase at 1e-4, the sampler kwargs of every block (cond_mask zeros, then ones), and case F's failure at block 1 of (2)."""
    from oracle import unet_ref
    from mcvd_pytorch_amd import runner as r
    g = task_fixture(golden_dir, case)
    cfg = task_config(g)
    X = task_batch(cfg, g)
    net = unet_ref.OracleScoreNet(cfg, synth.make_state_dict(cfg, seed=123))
    net.device = torch.device("cpu")
    for task, _ in r.video_tasks(cfg):
        _, cond, cond_mask, nfp = r.task_conditioning(cfg, X, task)
        idx, seen = task_calls(g, task), []
        kw = g["call_kwargs"][idx[0]]
        run = lambda: r.video_gen(cfg, net, cond, sampler=_oracle_sampler(g, idx, net, seen), task=task, cond_mask=cond_mask,   # noqa: E731
                                  verbose=kw["verbose"], log=kw["log"], init_noise_fn=lambda i, shp, dev: task_init(g, idx, i, shp))
        if g["error"] and g["error"]["phase"] == task:
            with pytest.raises(RuntimeError, match=f"left {g['error']['cond_channels']} cond channels"):
                run()
            assert len(seen) == g["error"]["block"] == len(idx)                 # refused before the block the reference failed on
            continue
        pred = run()
        assert seen == idx
        want = g["pred_raw"][task]
        assert pred.shape == want.shape
        err = (pred - want).abs().max().item()
        assert err <= TOL, f"{case} {task}: block loop vs the real runner {err:.3e}"


def test_task_refusals():
    """interp runs one block (num_frames_pred <= num_frames); a task the layout cannot run is a ValueError."""
    from mcvd_pytorch_amd import runner as r
    cfg = synth.make_config("tiny_spade")
    net = type("N", (), {"device": torch.device("cpu")})()
    cond = torch.zeros(1, 6, 32, 32)
    with pytest.raises(ValueError, match="interp"):
        r.video_gen(cfg, net, cond, num_frames_pred=3, task="interp", sampler=lambda *a, **k: None)
    with pytest.raises(ValueError, match="unknown task"):
        r.task_conditioning(cfg, torch.zeros(1, 4, 3, 32, 32), "predict")
    with pytest.raises(ValueError, match="num_frames_future == 0"):
        r.task_conditioning(cfg, torch.zeros(1, 4, 3, 32, 32), "pred")
    with pytest.raises(ValueError, match="num_frames_future > 0"):
        r.task_conditioning(synth.make_config("tiny"), torch.zeros(1, 6, 1, 32, 32), "interp")
