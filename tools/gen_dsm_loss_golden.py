"""Golden vectors of the REAL denoising score-matching loss (losses/dsm.py:7-52) and of the REAL `NCSNRunner.test()`
(runners/ncsn_runner.py:2370-2430) -- build container only (needs the reference checkout).

    PYTHONDONTWRITEBYTECODE=1 python -m tools.gen_dsm_loss_golden

The real `anneal_dsm_score_estimation` runs on the CPU on the real `UNetMore_DDPM` (oracle.gen_golden.build_ref_net) with the synthetic
weights of oracle/synth.py.  Nothing of the reference is replaced; its draws are observed from the outside:
  * torch.randint -> records the labels (case A injects 0, 333, 666, 999);
  * torch.randn_like -> records z (the loss's draw, then the conditioning noise of a noise_in_cond forward);
  * Gamma.sample -> records the raw gamma draws g (the loss's, then the forward's conditioning draw);
  * the net's forward -> records perturbed_x and eps; `hook` -> the per-row losses.
The fp64 column: the same call restated in float64 (oracle.unet_ref.OracleScoreNet(dtype=torch.float64): the reference net does not run in
fp64) from the recorded fp32 z and conditioning noise; drift64[b] = |L32[b] - L64[b]| / L64[b].

Fixtures tests/golden/dsm_loss_<case>.pt:
    A  tiny, L2, labels 0 / 333 / 666 / 999           B  tiny_condemb, prob_mask_cond 0.5 masks, L1
    C  tiny_gamma (gamma + noise_in_cond)             D  tiny_spade_noisecond
    E  the all_frames failure message (tiny_allframes)
  keys: config_name, L1, gamma, x, cond, cond_mask, labels, z (standardised under gamma), g (raw gamma draw or None), cond_z (the
  conditioning noise the forward used, standardised, or None), perturbed_x, eps, loss_rows, mean, loss64, drift64, buffers (the net's
  schedule / gamma tables)
    R  the real NCSNRunner.test(): two checkpoints (written to a temp dir from synth seeds, states[0] != the EMA shadow, model.ema on), an
       in-memory get_dataset, three batches of 4 per checkpoint; keys: ckpts, seeds, clips, order [ckpt][batch] (the DataLoader's rows),
       labels, z, eps, loss (per batch, fp32), loss_rows, drift64, log_lines, means.  The checkpoints are not committed: the tests rebuild
       them from the seeds (dsm_checkpoint below).
"""
import argparse
import logging
import os
import sys
import tempfile
from unittest import mock

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import torch  # noqa: E402

from oracle import synth, unet_ref  # noqa: E402
from oracle.gen_golden import build_ref_net  # noqa: E402
from oracle.gen_runner_golden import REF, import_real_runner  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")

CASES = {
    "A": dict(name="tiny", B=4, labels=[0, 333, 666, 999]),
    "B": dict(name="tiny_condemb", B=4, L1=True, prob_mask_cond=0.5),
    "C": dict(name="tiny_gamma", B=4, gamma=True),
    "D": dict(name="tiny_spade_noisecond", B=4),
}
R_SEEDS = {100: (201, 202), 200: (301, 302)}      # ckpt -> (states[0] seed, EMA shadow seed)


def dsm_checkpoint(config, seeds):
    """The list NCSNRunner.train saves (:425-433): [model state_dict ('module.' keys), optimiser state, epoch, step, EMA shadow (bare keys)]."""
    s0, s1 = seeds
    model = {"module." + k: v for k, v in synth.make_state_dict(config, seed=s0).items()}
    return [model, {}, 1, 0, synth.make_state_dict(config, seed=s1)]


def runner_test_config():
    config = synth.make_config("tiny")
    config.device = torch.device("cpu")
    config.model.version = "DDPM"
    config.model.ema, config.model.ema_rate = True, 0.999
    config.data.dataset, config.data.num_workers = "StochasticMovingMNIST", 0
    config.data.prob_mask_cond, config.data.prob_mask_future = 0.0, 0.0
    config.training = argparse.Namespace(loss_type="a", L1=False)
    config.test = argparse.Namespace(begin_ckpt=100, end_ckpt=200, freq=100, batch_size=4)
    return config


def _import_dsm():
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import losses.dsm as D
    return D


class _Spy:
    """Observes torch.randint / torch.randn_like / Gamma.sample during one reference call (optionally injecting the labels)."""

    def __init__(self, labels=None):
        self.labels, self.randint, self.randn, self.gamma = labels, [], [], []
        self._randint, self._randn_like = torch.randint, torch.randn_like
        from torch.distributions.gamma import Gamma
        self._sample = Gamma.sample

    def __enter__(self):
        from torch.distributions.gamma import Gamma
        spy = self

        def randint(*a, **kw):
            out = spy._randint(*a, **kw)
            if spy.labels is not None:
                out = torch.tensor(spy.labels, dtype=out.dtype, device=out.device)
            spy.randint.append(out.clone())
            return out

        def randn_like(like, *a, **kw):
            out = spy._randn_like(like, *a, **kw)
            spy.randn.append(out.clone())
            return out

        def sample(self_, *a, **kw):
            out = spy._sample(self_, *a, **kw)
            spy.gamma.append(out.clone())
            return out
        self._patches = [mock.patch.object(torch, "randint", randint), mock.patch.object(torch, "randn_like", randn_like),
                         mock.patch.object(Gamma, "sample", sample)]
        for p in self._patches:
            p.start()
        return self

    def __exit__(self, *exc):
        for p in self._patches:
            p.stop()


def _spy_forward(net, rec):
    real = net.forward

    def forward(x, y, cond=None, cond_mask=None):
        out = real(x, y, cond=cond, cond_mask=cond_mask)
        rec.append((x.clone(), out.clone()))
        return out
    net.forward = forward


def _standardise(g, labels, net, like):
    """(g - k_cum theta_t) / sqrt(1 - alpha) exactly as losses/dsm.py:31-34 and ncsnpp_more.py:762-765 evaluate it."""
    B = like.shape[0]
    ua = net.alphas[labels].reshape(B, *([1] * len(like.shape[1:])))
    uk = net.k_cum[labels].reshape(B, *([1] * len(like.shape[1:]))).repeat(1, *like.shape[1:])
    ut = net.theta_t[labels].reshape(B, *([1] * len(like.shape[1:]))).repeat(1, *like.shape[1:])
    return (g - uk * ut) / (1 - ua).sqrt()


def loss64(config, sd, x, labels, z, cond, cond_mask, cond_z, L1):
    """The same call in float64 from the fp32 z / conditioning noise: perturbation, OracleScoreNet(float64), reduction."""
    net64 = unet_ref.OracleScoreNet(config, sd, dtype=torch.float64)
    if cond_z is not None:
        net64.cond_noise_fn = lambda c: cond_z.double()
    a = net64.alphas[labels].reshape(-1, 1, 1, 1)
    px = a.sqrt() * x.double() + (1 - a).sqrt() * z.double()
    eps = net64(px, labels, cond=cond.double() if cond is not None else None, cond_mask=cond_mask)
    d = z.double() - eps
    t = d.abs() if L1 else 0.5 * d.square()
    return t.reshape(len(x), -1).sum(dim=-1)


def gen_case(tag, name, B, L1=False, gamma=False, prob_mask_cond=0.0, labels=None):
    D = _import_dsm()
    config = synth.make_config(name)
    net = build_ref_net(config)
    sd = synth.make_state_dict(config, seed=123)
    net.load_state_dict(sd, strict=False)
    x, cond = synth.make_inputs(config, B, seed=5)
    cond_mask = None
    if prob_mask_cond > 0:                                  # conditioning_fn's mask (runners/ncsn_runner.py:120-123)
        keep = torch.rand(B, generator=torch.Generator().manual_seed(9)) > prob_mask_cond
        cond = keep.reshape(-1, 1, 1, 1) * cond
        cond_mask = keep.to(torch.int32)
    rec, rows = [], []
    _spy_forward(net, rec)
    torch.manual_seed(1000 + ord(tag))
    with _Spy(labels) as spy, torch.no_grad():
        mean = D.anneal_dsm_score_estimation(net, x, labels=None, cond=cond, cond_mask=cond_mask, gamma=gamma, L1=L1,
                                             hook=lambda loss, lab: rows.append(loss.clone()))
    lab = spy.randint[0]
    assert len(spy.randint) == 1 and len(rec) == 1 and len(rows) == 1
    px, eps = rec[0]
    nic = bool(config.model.noise_in_cond)
    g = cond_z = None
    if gamma:
        assert len(spy.gamma) == (2 if nic else 1) and not spy.randn
        g = spy.gamma[0]
        z = _standardise(g, lab, net, x)
        if nic:
            cond_z = _standardise(spy.gamma[1], lab, net, cond)
    else:
        assert len(spy.randn) == (2 if nic else 1) and not spy.gamma
        z = spy.randn[0]
        if nic:
            cond_z = spy.randn[1]
    a = net.alphas[lab].reshape(B, 1, 1, 1)
    assert torch.equal(a.sqrt() * x + (1 - a).sqrt() * z, px)              # the recorded z is the one the reference used
    l64 = loss64(config, sd, x, lab, z, cond, cond_mask, cond_z, L1)
    drift = ((rows[0].double() - l64).abs() / l64).tolist()
    bufs = {k: v.clone() for k, v in net.state_dict().items() if k in ("betas", "alphas", "alphas_prev", "k", "k_cum", "theta_t")}
    out = dict(config_name=name, L1=L1, gamma=gamma, x=x, cond=cond, cond_mask=cond_mask, labels=lab, z=z, g=g, cond_z=cond_z,
               perturbed_x=px, eps=eps, loss_rows=rows[0], mean=mean, loss64=l64, drift64=drift, buffers=bufs)
    torch.save(out, os.path.join(OUT, f"dsm_loss_{tag}.pt"))
    print(f"dsm_loss_{tag}.pt: {name} labels {lab.tolist()} loss {rows[0].tolist()} mean {mean.item():.6g} drift64 {max(drift):.2e}")


def gen_allframes():
    D = _import_dsm()
    config = synth.make_config("tiny_allframes")
    net = build_ref_net(config)
    net.load_state_dict(synth.make_state_dict(config, seed=123), strict=False)
    x, cond = synth.make_inputs(config, 2, seed=5)
    try:
        with torch.no_grad():
            D.anneal_dsm_score_estimation(net, x, cond=cond, all_frames=True)
        raise AssertionError("all_frames=True did not fail")
    except RuntimeError as e:
        msg = str(e)
    torch.save(dict(config_name="tiny_allframes", message=msg), os.path.join(OUT, "dsm_loss_E.pt"))
    print(f"dsm_loss_E.pt: {msg}")


def gen_runner():
    R = import_real_runner()
    config = runner_test_config()
    C, S = config.data.channels, config.data.image_size
    T = config.data.num_frames_cond + config.data.num_frames
    n_clips, B = 12, config.test.batch_size
    clips = torch.rand(n_clips, T, C, S, S, generator=torch.Generator().manual_seed(41))
    ds = torch.utils.data.TensorDataset(clips, torch.zeros(n_clips))
    tmp = tempfile.mkdtemp(prefix="mcvd_dsm_")
    for ckpt, seeds in R_SEEDS.items():
        torch.save(dsm_checkpoint(config, seeds), os.path.join(tmp, f"checkpoint_{ckpt}.pt"))
    args = argparse.Namespace(log_path=tmp, data_path=tmp)
    runner = R.NCSNRunner(args, config, None)
    real_loss, calls = R.anneal_dsm_score_estimation, []

    def loss_spy(scorenet, x, **kw):
        rec, call = [], {}
        net = scorenet.module
        _spy_forward(net, rec)
        with _Spy() as spy:
            out = real_loss(scorenet, x, hook=lambda loss, lab: call.update(rows=loss.clone()), **kw)
        del net.forward
        call.update(x=x.clone(), labels=spy.randint[0], z=spy.randn[0], eps=rec[0][1], loss=out.clone(),
                    kw={k: v for k, v in kw.items() if not torch.is_tensor(v)})
        calls.append(call)
        return out
    lines = []
    handler = logging.Handler()
    handler.emit = lambda r: lines.append(r.getMessage())
    logging.getLogger().addHandler(handler)
    logging.getLogger().setLevel(logging.INFO)
    torch.manual_seed(77)
    with mock.patch.object(R, "get_dataset", lambda *a, **kw: (ds, ds)), mock.patch.object(R, "anneal_dsm_score_estimation", loss_spy):
        runner.test()
    logging.getLogger().removeHandler(handler)
    log_lines = [ln for ln in lines if ln.startswith("ckpt: ")]
    ckpts = list(R_SEEDS)
    nb = n_clips // B
    assert len(calls) == nb * len(ckpts) and len(log_lines) == len(ckpts), (len(calls), log_lines)
    dt = R.data_transform(config, clips)
    order, drift, l64s = [], [], []
    for k, c in enumerate(calls):
        ckpt = ckpts[k // nb]
        pred = dt.flatten(1, 2)[:, C * config.data.num_frames_cond:]
        order.append([int((pred - c["x"][r]).flatten(1).abs().max(dim=1).values.argmin()) for r in range(B)])
        shadow = dsm_checkpoint(config, R_SEEDS[ckpt])[-1]
        cond = dt[order[-1]][:, :config.data.num_frames_cond].flatten(1, 2)
        l64 = loss64(config, shadow, c["x"], c["labels"], c["z"], cond, None, None, False)
        l64s.append(l64)
        drift.append(((c["rows"].double() - l64).abs() / l64).tolist())
    means = [float(ln.split("average test loss: ")[1]) for ln in log_lines]
    out = dict(config_name="tiny", ckpts=ckpts, seeds=R_SEEDS, clips=clips, batch=B, order=[order[i:i + nb] for i in range(0, len(order), nb)],
               labels=[c["labels"] for c in calls], z=[c["z"] for c in calls], eps=[c["eps"] for c in calls],
               loss=[c["loss"] for c in calls], loss_rows=[c["rows"] for c in calls], loss64=l64s, drift64=drift, log_lines=log_lines,
               means=means, kwargs=calls[0]["kw"])
    torch.save(out, os.path.join(OUT, "dsm_loss_R.pt"))
    print(f"dsm_loss_R.pt: {log_lines}, order {out['order']}, max drift64 {max(max(d) for d in drift):.2e}")


if __name__ == "__main__":
    torch.set_num_threads(8)
    which = sys.argv[1:] or list(CASES) + ["E", "R"]
    for tag in which:
        if tag in CASES:
            gen_case(tag, **CASES[tag])
        elif tag == "E":
            gen_allframes()
        elif tag == "R":
            gen_runner()
