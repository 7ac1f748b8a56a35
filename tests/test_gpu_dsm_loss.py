"""GPU: the denoising score-matching loss on the device -- mcvd_dsm_loss (kernels/dsm.cpp) through dsm_loss_rows /
anneal_dsm_score_estimation / test_checkpoints -- against the REAL reference's fixtures (tests/golden/dsm_loss_*.pt, cases in
tests/test_dsm_loss_cpu.py) and against the CPU oracle at config 2's shape under the committed kernel table.

Gates: perturbation bit-exact (torch's fp32 CPU expression); reduction = the fp64 sum of the fp32 terms rounded once, or 1 fp32 ulp off
(the fp64 summation-order difference is <= N 2^-53 sum|t|, far below half an ulp: only a tie can flip the rounding); parity with the
reference per row and for the mean: tests/dsm_ref.py row_gates (DESIGN section 3's forward contract carried through the loss)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import synth, unet_ref
from tests import dsm_ref
from tests.test_dsm_loss_cpu import CASES, ServedBatches, fixture, write_checkpoints

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(name, buffers=None, config=None):
    from mcvd_pytorch_amd import HipScoreNet
    config = config or synth.make_config(name)
    config.device = "cuda:0"
    net = HipScoreNet(config)
    net.load_state_dict({**synth.make_state_dict(config, seed=123), **(buffers or {})}, strict=True)
    return config, net.eval()


def _cuda(t):
    return t.cuda() if t is not None else None


def _run(net, g, **kw):
    """dsm_loss_rows on the fixture's x, labels, cond, mask and z (the raw gamma draw under gamma), with its conditioning noise."""
    from mcvd_pytorch_amd.losses import dsm_loss_rows
    if g["cond_z"] is not None:
        net.set_next_cond_noise(g["cond_z"].cuda())
    return dsm_loss_rows(net, g["x"].cuda(), g["labels"].cuda(), cond=_cuda(g["cond"]), cond_mask=_cuda(g["cond_mask"]), gamma=g["gamma"],
                         L1=g["L1"], z=(g["g"] if g["gamma"] else g["z"]).cuda(), return_z=True, return_perturbed=True, **kw)


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


@pytest.mark.parametrize("case", CASES)
def test_perturbation_is_exact(golden_dir, case):
    """perturbed_out is the reference's perturbed_x bit for bit, and z_out its z (case C: the standardisation of the injected raw g)."""
    g = fixture(golden_dir, case)
    _, net = _net(g["config_name"], g["buffers"])
    _, z, px = _run(net, g)
    assert torch.equal(z.cpu(), g["z"])
    assert torch.equal(px.cpu(), g["perturbed_x"])


@pytest.mark.parametrize("case", CASES)
def test_reduction(golden_dir, case):
    """Every row equals the fp64 host sum of the fp32 terms of the device's own z and eps, rounded to fp32, or is 1 ulp off."""
    g = fixture(golden_dir, case)
    _, net = _net(g["config_name"], g["buffers"])
    loss, z, px = _run(net, g)
    if g["cond_z"] is not None:
        net.set_next_cond_noise(g["cond_z"].cuda())
    eps = net(px, g["labels"].cuda(), cond=_cuda(g["cond"]), cond_mask=_cuda(g["cond_mask"]))        # the same forward again: bit-identical
    want = dsm_ref.terms32_sum64(z.cpu(), eps.cpu(), g["L1"]).float().numpy()
    d = np.abs(loss.cpu().double().numpy() - want.astype(np.float64))
    print(f"  {case}: |device - host| / ulp {(d / _ulp32(want)).tolist()}")
    assert np.all(d <= _ulp32(want))


@pytest.mark.parametrize("case", CASES)
def test_parity_with_the_reference(golden_dir, case):
    g = fixture(golden_dir, case)
    _, net = _net(g["config_name"], g["buffers"])
    loss, _, _ = _run(net, g)
    gate = dsm_ref.row_gates(g["z"], g["eps"], g["loss_rows"], max(g["drift64"]), g["L1"])
    d = (loss.cpu().double() - g["loss_rows"].double()).abs()
    dm = abs(loss.mean().item() - g["mean"].item())
    print(f"  {case}: per-row |dL| {d.tolist()} gate {gate.tolist()}; mean |dL| {dm:.4e} gate {gate.mean().item():.4e}")
    assert torch.all(d <= gate)
    assert dm <= gate.mean().item()


def test_config2_under_the_committed_table():
    """What the bench runs: config 2 at B = 64 under profiles/tune_smmnist_big5_ngf96_B64_bf16x3.json, synthetic weights, injected labels and
    z; rows 0 and 63 against OracleScoreNet (fp32 CPU, B = 2) under row_gates.  The oracle's loss is summed in fp64, so its drift term is
    the fp32 rounding of the device's terms and row alone: drift64 = 2^-22 (four fp32 roundings, relative).  Every conv op ran the kernel the
    table names (mcvd_model_op_kernel)."""
    from mcvd_pytorch_amd import _lib
    from mcvd_pytorch_amd.losses import dsm_loss_rows
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    config, net = _net("smmnist_big5_ngf96")
    B = 64
    table = json.load(open(os.path.join(ROOT, "profiles", "tune_smmnist_big5_ngf96_B64_bf16x3.json")))[str(B)]
    net.set_tuning(B, table)
    x, cond = synth.make_inputs(config, B, seed=0)
    labels = torch.linspace(0, 999, B).long()
    z = torch.randn(x.shape, generator=torch.Generator().manual_seed(3))
    loss, _, _ = dsm_loss_rows(net, x.cuda(), labels.cuda(), cond=cond.cuda(), z=z.cuda())
    info = (C.c_int * 8)()
    n = _lib.lib.mcvd_model_profile_read(net._model, None, None, None, None, None, 0)
    assert n == len(table)
    ran = 0
    for i in range(n):
        _lib.check(_lib.lib.mcvd_model_op_info(net._model, i, info), "op_info")
        if info[0] != 3 or table[i][0] < 0:
            continue
        k = _lib.lib.mcvd_model_op_kernel(net._model, i)
        assert k == table[i][0], f"op {i}: ran kernel {k}, the table names {table[i][0]}"
        ran += 1
    assert ran > 50
    oracle = unet_ref.OracleScoreNet(config, synth.make_state_dict(config, seed=123))
    rows = [0, B - 1]
    px = dsm_ref.perturb32(x[rows], labels[rows], oracle.alphas, z[rows])
    eps = oracle(px, labels[rows], cond=cond[rows])
    ref = dsm_ref.loss_rows64(z[rows], eps)
    gate = dsm_ref.row_gates(z[rows], eps, ref, 2.0 ** -22)
    d = (loss.cpu()[rows].double() - ref).abs()
    print(f"  config 2, B = 64, rows {rows}: |dL| {d.tolist()} gate {gate.tolist()}")
    assert torch.all(d <= gate)


def test_device_draws_and_shard_invariance():
    """z = None: the device's z equals mcvd_randn's layout for the documented key (seed, sample_offset + row, draw 2^40) bit for bit; rows 3-4
    of a B = 5 call equal a B = 2 call with sample_offset = 3 in z and in loss, under one kernel table."""
    from mcvd_pytorch_amd.losses import dsm_loss_rows
    from tests.hiputil import Ctx
    config, net = _net("tiny")
    x, cond = synth.make_inputs(config, 5, seed=1)
    labels = torch.tensor([5, 100, 400, 777, 999])
    l5, z5, _ = dsm_loss_rows(net, x.cuda(), labels.cuda(), cond=cond.cuda(), seed=11, return_z=True)
    per = z5[0].numel()
    want = Ctx().randn(5, per, 11, 0, 1 << 40)
    assert torch.equal(z5.reshape(5, per), want)
    net.set_tuning(2, net.get_tuning(5))
    l2, z2, _ = dsm_loss_rows(net, x[3:].cuda(), labels[3:].cuda(), cond=cond[3:].cuda(), seed=11, sample_offset=3, return_z=True)
    assert torch.equal(z2, z5[3:]) and torch.equal(l2, l5[3:])


def _moments(z, sd):
    v = (z.double() / sd.reshape(-1, 1, 1, 1)).flatten()
    n = v.numel()
    return n, v.mean().item(), v.var(unbiased=False).item()


@pytest.mark.parametrize("gamma", [False, True], ids=["normal", "gamma"])
def test_draw_moments(gamma):
    """B = 64 rows of 20 480 elements, labels linspace(0, 999, 64), z drawn on the device, each row divided by its expected standard deviation
    (1; gamma: sqrt(k_cum theta_t^2 / (1 - alpha)) from the tables): |mean| <= 6 / sqrt(n) and |var - 1| <= 6 sqrt(2 / n) over the pool."""
    from mcvd_pytorch_amd.losses import dsm_loss_rows
    config = synth.make_config("tiny_gamma" if gamma else "tiny")
    config.data.image_size, config.data.num_frames = 64, 5                # 20 480 elements per row, as config 2
    _, net = _net(None, config=config)
    net.set_option("autotune", 0)
    B = 64
    x, cond = synth.make_inputs(config, B, seed=2)
    labels = torch.linspace(0, 999, B).long()
    _, z, _ = dsm_loss_rows(net, x.cuda(), labels.cuda(), cond=cond.cuda(), gamma=gamma, seed=21, return_z=True)
    if gamma:
        k, th, a = (t.cpu().double()[labels] for t in (net.k_cum, net.theta_t, net.alphas))
        sd = (k * th * th / (1 - a)).sqrt()
    else:
        sd = torch.ones(B, dtype=torch.float64)
    n, m, v = _moments(z.cpu(), sd)
    print(f"  {'gamma' if gamma else 'normal'}: n {n}, mean {m:.3e} (cap {6 / math.sqrt(n):.2e}), var - 1 {v - 1:.3e} (cap {6 * math.sqrt(2 / n):.2e})")
    assert abs(m) <= 6 / math.sqrt(n)
    assert abs(v - 1) <= 6 * math.sqrt(2 / n)


def test_runner_against_the_real_test_mode(golden_dir, tmp_path):
    """test_checkpoints on fixture R's checkpoints (rebuilt from the seeds), served batches, labels and z: the per-checkpoint means within the
    mean of the row gates of their batches, the log lines in the reference's text, and the EMA shadow -- not states[0] -- in the net."""
    from mcvd_pytorch_amd import anneal_dsm_score_estimation, get_model
    from mcvd_pytorch_amd.runner import test_checkpoints as run_checkpoints
    from tools.gen_dsm_loss_golden import dsm_checkpoint, runner_test_config
    g = fixture(golden_dir, "R")
    config = runner_test_config()
    config.device = "cuda:0"
    write_checkpoints(g, config, str(tmp_path))
    net = get_model(config)
    k = [0]

    def loss_fn(scorenet, x, **kw):
        i = k[0]
        k[0] += 1
        kw["labels"] = g["labels"][i].cuda()
        return anneal_dsm_score_estimation(scorenet, x, z=g["z"][i].cuda(), **kw)
    lines = []
    means = run_checkpoints(config, net, ServedBatches(g), str(tmp_path), loss_fn=loss_fn, log=lines.append)
    nb = len(g["order"][0])
    for c, ckpt in enumerate(g["ckpts"]):
        gates = [dsm_ref.row_gates(g["z"][i], g["eps"][i], g["loss_rows"][i], max(g["drift64"][i])).mean().item()
                 for i in range(c * nb, (c + 1) * nb)]
        gate = sum(gates) / nb
        d = abs(means[ckpt] - g["means"][c])
        print(f"  ckpt {ckpt}: mean {means[ckpt]!r} vs {g['means'][c]!r}, |d| {d:.4e}, gate {gate:.4e}")
        assert d <= gate
        head, num = lines[c].rsplit(" ", 1)
        want_head, want_num = g["log_lines"][c].rsplit(" ", 1)
        assert head == want_head == f"ckpt: {ckpt}, average test loss:" and abs(float(num) - float(want_num)) <= gate
    shadow, states0 = dsm_checkpoint(config, g["seeds"][g["ckpts"][-1]])[-1], dsm_checkpoint(config, g["seeds"][g["ckpts"][-1]])[0]
    for name, p in net.named_parameters():
        assert torch.equal(p.data.cpu(), shadow[name]) and not torch.equal(p.data.cpu(), states0["module." + name])


def test_deterministic():
    from mcvd_pytorch_amd.losses import dsm_loss_rows
    config, net = _net("tiny_condemb")
    x, cond = synth.make_inputs(config, 4, seed=3)
    labels, mask = torch.tensor([1, 500, 900, 999]).cuda(), torch.tensor([1, 0, 1, 0], dtype=torch.int32).cuda()
    a = dsm_loss_rows(net, x.cuda(), labels, cond=cond.cuda(), cond_mask=mask, L1=True, seed=5)[0]
    b = dsm_loss_rows(net, x.cuda(), labels, cond=cond.cuda(), cond_mask=mask, L1=True, seed=5)[0]
    c = dsm_loss_rows(net, x.cuda(), labels, cond=cond.cuda(), cond_mask=mask, L1=True, seed=6)[0]
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_abi_errors():
    """MCVD_DSM_GAMMA without gamma tables, an unknown flag and a NULL loss buffer: MCVD_EINVAL; the valid call returns 0."""
    from mcvd_pytorch_amd import _lib
    config, net = _net("tiny")
    x, cond = synth.make_inputs(config, 2, seed=0)
    x, cond = x.cuda(), cond.cuda()
    labels = torch.tensor([1, 2]).cuda()
    loss = torch.empty(2, device="cuda")
    net.sync_parameters()
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    call = lambda flags, out: _lib.lib.mcvd_dsm_loss(net._model, P(x), P(labels), P(cond), None, None, 1, 0, flags, P(out), None, None, 2)  # noqa: E731
    assert call(_lib.DSM_GAMMA, loss) == -1 and "gamma tables" in _lib.last_error()
    assert call(4, loss) == -1
    assert call(0, None) == -1
    assert call(_lib.DSM_L1, loss) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
