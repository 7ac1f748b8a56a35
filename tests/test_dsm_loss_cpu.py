"""CPU: the denoising score-matching loss of NCSNRunner.test() (losses/dsm.py:7-52, runners/ncsn_runner.py:2370-2430) against the fixtures
the REAL reference wrote (tools/gen_dsm_loss_golden.py):

    A  tiny, L2, labels 0 / 333 / 666 / 999        B  tiny_condemb, prob_mask_cond 0.5 masks, L1
    C  tiny_gamma (gamma + noise_in_cond)          D  tiny_spade_noisecond
    E  the all_frames failure message              R  the real NCSNRunner.test(): two checkpoints, EMA, three batches of 4

tests/dsm_ref.py restates the reduction in fp64; OracleScoreNet restates the forward; the argument handling and the runner loop of
mcvd_pytorch_amd run on a plan-only HipScoreNet (no GPU)."""
import os

import pytest
import torch

from oracle import synth, unet_ref
from tests import dsm_ref
from tests.golden_io import load_golden

CASES = ["A", "B", "C", "D"]


def fixture(golden_dir, case):
    return load_golden(golden_dir, f"dsm_loss_{case}.pt")


def write_checkpoints(g, config, path):
    """Fixture R's checkpoints, rebuilt from their seeds into `path`."""
    from tools.gen_dsm_loss_golden import dsm_checkpoint
    for ckpt in g["ckpts"]:
        torch.save(dsm_checkpoint(config, g["seeds"][ckpt]), os.path.join(path, f"checkpoint_{ckpt}.pt"))


class ServedBatches:
    """Fixture R's DataLoader: the clips it served for each checkpoint, in its order; one pass per checkpoint."""

    def __init__(self, g):
        self.g, self.k = g, 0

    def __iter__(self):
        order = self.g["order"][self.k]
        self.k += 1
        for rows in order:
            yield self.g["clips"][rows], torch.zeros(len(rows))


@pytest.mark.parametrize("case", CASES)
def test_restated_reduction_reproduces_the_reference(golden_dir, case):
    """The fp64 sum of the recorded z and eps reproduces each per-row loss within 3 x the recorded fp32-vs-fp64 distance of the call, and the
    recorded mean is the fp32 mean of the rows."""
    g = fixture(golden_dir, case)
    got = dsm_ref.loss_rows64(g["z"], g["eps"], g["L1"])
    ref = g["loss_rows"].double()
    gate = 3 * max(g["drift64"]) * ref
    print(f"  {case}: max |dL| / L {((got - ref).abs() / ref).max().item():.2e}, gate {3 * max(g['drift64']):.2e}")
    assert torch.all((got - ref).abs() <= gate)
    assert torch.equal(g["loss_rows"].mean(dim=0), g["mean"])


@pytest.mark.parametrize("case", CASES)
def test_perturbation_restatement_is_bit_exact(golden_dir, case):
    """sqrt(a) x + sqrt(1 - a) z in torch fp32 from the fixture's own tables is the reference's perturbed_x bit for bit (the device is held to
    the same expression)."""
    g = fixture(golden_dir, case)
    assert torch.equal(dsm_ref.perturb32(g["x"], g["labels"], g["buffers"]["alphas"], g["z"]), g["perturbed_x"])


@pytest.mark.parametrize("case", CASES)
def test_oracle_forward_reproduces_eps(golden_dir, case):
    """OracleScoreNet on the fixture's perturbed_x (with its conditioning noise and masks) reproduces the reference's eps within the
    project's forward gate, 1e-4 max|eps|."""
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    g = fixture(golden_dir, case)
    config = synth.make_config(g["config_name"])
    net = unet_ref.OracleScoreNet(config, synth.make_state_dict(config, seed=123))
    if g["cond_z"] is not None:
        net.cond_noise_fn = lambda c: g["cond_z"]
    eps = net(g["perturbed_x"], g["labels"], cond=g["cond"], cond_mask=g["cond_mask"])
    assert (eps - g["eps"]).abs().max().item() <= 1e-4 * g["eps"].abs().max().item()


def test_argument_handling_on_a_plan_only_net(golden_dir):
    """SMLD -> NotImplementedError; all_frames -> the reference's message (fixture E) before any device work; mis-shaped x, labels, cond and z
    -> RuntimeError; gamma=True on a net without gamma tables -> AttributeError, as the reference's `net.k_cum`."""
    from mcvd_pytorch_amd import HipScoreNet, anneal_dsm_score_estimation
    from mcvd_pytorch_amd.losses import dsm_loss_rows
    config = synth.make_config("tiny")
    net = HipScoreNet(config, plan_only=True)
    x, cond = synth.make_inputs(config, 2, seed=0)
    lab = torch.tensor([3, 4])
    smld = synth.make_config("tiny")
    smld.model.version = "SMLD"
    with pytest.raises(NotImplementedError):
        anneal_dsm_score_estimation(HipScoreNet(smld, plan_only=True), x, cond=cond)
    e = fixture(golden_dir, "E")
    af = synth.make_config(e["config_name"])
    xa, ca = synth.make_inputs(af, 2, seed=5)
    with pytest.raises(RuntimeError) as err:
        anneal_dsm_score_estimation(HipScoreNet(af, plan_only=True), xa, cond=ca, all_frames=True)
    assert str(err.value) == e["message"]
    with pytest.raises(RuntimeError, match="x has shape"):
        dsm_loss_rows(net, x[:, :1], lab, cond=cond)
    with pytest.raises(RuntimeError, match="labels have shape"):
        dsm_loss_rows(net, x, lab[:1], cond=cond)
    with pytest.raises(RuntimeError, match="cond missing"):
        dsm_loss_rows(net, x, lab, cond=None)
    with pytest.raises(RuntimeError, match="z has shape"):
        dsm_loss_rows(net, x, lab, cond=cond, z=x[:1])
    with pytest.raises(AttributeError, match="k_cum"):
        anneal_dsm_score_estimation(net, x, cond=cond, gamma=True)
    with pytest.raises(RuntimeError, match="plan_only"):
        dsm_loss_rows(net, x, lab, cond=cond)


def test_runner_loop_against_the_real_test_mode(golden_dir, tmp_path):
    """test_checkpoints fed fixture R's per-batch values: the checkpoint range of the config, the reference's mean arithmetic and log lines
    exactly, the reference's keywords to the loss, and the EMA shadow (not states[0]) in the net's parameters afterwards."""
    from mcvd_pytorch_amd import HipScoreNet
    from mcvd_pytorch_amd.runner import data_transform, test_checkpoints as run_checkpoints
    from tools.gen_dsm_loss_golden import dsm_checkpoint, runner_test_config
    g = fixture(golden_dir, "R")
    config = runner_test_config()
    write_checkpoints(g, config, str(tmp_path))
    net = HipScoreNet(config, plan_only=True)
    seen, lines = [], []

    def loss_fn(scorenet, x, **kw):
        k = len(seen)
        seen.append(kw)
        want = data_transform(config, g["clips"][g["order"][k // 3][k % 3]]).flatten(1, 2)[:, config.data.num_frames_cond * config.data.channels:]
        assert torch.equal(x, want)
        return g["loss"][k]
    means = run_checkpoints(config, net, ServedBatches(g), str(tmp_path), loss_fn=loss_fn, log=lines.append)
    assert list(means) == g["ckpts"] == [100, 200]
    assert lines == g["log_lines"]
    assert [means[c] for c in g["ckpts"]] == g["means"]
    assert len(seen) == 6 and all({k: v for k, v in kw.items() if not torch.is_tensor(v)} == g["kwargs"] for kw in seen)
    shadow = dsm_checkpoint(config, g["seeds"][200])[-1]
    states0 = dsm_checkpoint(config, g["seeds"][200])[0]
    for name, p in net.named_parameters():
        assert torch.equal(p.data, shadow[name]) and not torch.equal(p.data, states0["module." + name])
