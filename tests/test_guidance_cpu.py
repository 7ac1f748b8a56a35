"""CPU: classifier-free guidance without the library.

  * `runner.guidance_conditioning` on hand-built tensors (the concat and the SPADE layouts);
  * the fixture tests/golden/guidance.pt (tools/gen_guidance_golden.py: the REAL reference samplers over a wrapped real net) is reproduced
    by the oracle's restated samplers over a guided wrapper of the oracle's net, under the gate tests/test_oracle_golden.py applies to a
    sampler output that travels with its fp32-vs-fp64 distance: max(1e-4, 3 x that distance);
  * the fixture's scale-1 cases equal the reference's unguided runs of the same inputs bit for bit (e_c + 0 * (e_c - e_u) is e_c)."""
import pytest
import torch

from oracle import sampler_ref, synth, unet_ref
from tests.golden_io import load_golden

N_CASES = 13


@pytest.fixture(scope="module")
def fx(golden_dir):
    return load_golden(golden_dir, "guidance.pt")


class GuidedOracle:
    """The samplers' `scorenet`: e_c + (s - 1) * (e_c - e_u) over the oracle's net."""

    def __init__(self, net, scale, cond_weak, mask):
        self.net, self.scale, self.cond_weak, self.mask = net, scale, cond_weak, mask
        self.alphas, self.alphas_prev, self.betas = net.alphas, net.alphas_prev, net.betas

    def __call__(self, x, t, cond=None):
        e_c = self.net(x, t, cond=cond)
        mask = torch.full((x.shape[0],), self.mask, dtype=torch.int32) if self.net.c.cond_emb else None
        e_u = self.net(x, t, cond=self.cond_weak, cond_mask=mask)
        return e_c + (self.scale - 1) * (e_c - e_u)


def case_tensors(g, c):
    name = c["config_name"]
    return (g[f"x_init.{name}"], g[f"cond.{name}"], g[f"cond_weak.{name}.{c['drop']}"], g[f"noise.{name}"], g[f"result.{name}"][c["row"]],
            g[f"result64.{name}"][c["row"]])


def test_fixture_holds_the_cases_of_the_issue(fx):
    got = sorted((c["config_name"], c["drop"], c["kind"], c["scale"], c["t_min"]) for c in fx["cases"])
    want = sorted([("tiny", "all", k, s, -1) for k in ("ddpm", "ddim", "fpndm") for s in (0.0, 1.0, 2.5)] +
                  [("tiny_condemb", "all", "ddpm", 2.5, -1), ("tiny_spade", "past", "ddpm", 2.5, -1),
                   ("tiny_spade", "future", "ddpm", 2.5, -1), ("tiny", "all", "ddpm", 2.5, 0.3)])
    assert got == want and len(got) == N_CASES
    assert fx["batch"] == 2 and fx["subsample"] == 10
    for c in fx["cases"]:
        x, cond, weak, noise, res, res64 = case_tensors(fx, c)
        assert weak.shape == cond.shape and res.shape == (1,) + x.shape and res64.dtype == torch.float64
        assert c["ref_dev"] == float((res.double() - res64).abs().max())
        assert c["mask"] == (1 if c["drop"] == "future" else 0)


@pytest.mark.parametrize("i", range(N_CASES))
def test_oracle_reproduces_the_guided_reference(fx, i):
    c = fx["cases"][i]
    x, cond, weak, noise, res, _ = case_tensors(fx, c)
    config = synth.make_config(c["config_name"])
    net = GuidedOracle(unet_ref.OracleScoreNet(config, synth.make_state_dict(config, seed=123)), c["scale"], weak, c["mask"])
    if c["kind"] == "fpndm":
        out = sampler_ref.fpndm_sample(x.clone(), net, cond=cond, final_only=True, subsample_steps=fx["subsample"], clip_before=True)
    else:
        k = [0]

        def fn(_, like):
            k[0] += 1
            return noise[k[0] - 1]
        kw = dict(t_min=c["t_min"]) if c["t_min"] > 0 else {}
        out = sampler_ref.sample(x.clone(), net, cond=cond, kind=c["kind"], final_only=True, denoise=True, subsample_steps=fx["subsample"],
                                 clip_before=True, noise_fn=fn, **kw)
        assert k[0] == c["n_noise"]
    err, gate = (out - res).abs().max().item(), max(1e-4, 3.0 * c["ref_dev"])
    print(f"{c['id']}: err {err:.3e}, gate {gate:.3e}")
    assert err <= gate, f"{c['id']}: {err:.3e} > {gate:.3e}"


@pytest.mark.parametrize("kind", ["ddpm", "ddim", "fpndm"])
def test_scale_one_is_the_unguided_reference_run(fx, kind):
    (c,) = [c for c in fx["cases"] if c["config_name"] == "tiny" and c["kind"] == kind and c["scale"] == 1.0]
    res = fx["result.tiny"][c["row"]]
    assert torch.equal(res, fx["unguided"][kind])
    other = fx["result.tiny"][[d for d in fx["cases"] if d["config_name"] == "tiny" and d["kind"] == kind and d["scale"] == 2.5
                               and d["t_min"] <= 0][0]["row"]]
    assert (other - res).abs().max().item() > 1e-2          # the scale moves the frames


def _config(name):
    return synth.make_config(name)


def test_guidance_conditioning_concat_layout():
    from mcvd_pytorch_amd.runner import guidance_conditioning
    config = _config("tiny")                                  # 2 past frames, no future block, 1 channel
    cond = torch.arange(1, 1 + 3 * 2 * 4 * 4, dtype=torch.float32).reshape(3, 2, 4, 4)
    keep = cond.clone()
    for drop in ("past", "all"):
        weak, mask = guidance_conditioning(config, cond, drop)
        assert mask == 0 and weak.shape == cond.shape and weak.dtype == cond.dtype and not weak.any()
        assert weak.data_ptr() != cond.data_ptr()
    assert torch.equal(cond, keep)
    with pytest.raises(ValueError, match="future"):
        guidance_conditioning(config, cond, "future")
    with pytest.raises(ValueError, match="unknown"):
        guidance_conditioning(config, cond, "none")
    with pytest.raises(ValueError, match="shape"):
        guidance_conditioning(config, cond[:, :1], "all")


def test_guidance_conditioning_spade_layout():
    from mcvd_pytorch_amd.runner import guidance_conditioning
    config = _config("tiny_spade")                            # 1 past frame | 1 future frame, 3 channels
    cond = torch.arange(1, 1 + 2 * 6 * 4 * 4, dtype=torch.float32).reshape(2, 6, 4, 4)
    keep = cond.clone()
    weak, mask = guidance_conditioning(config, cond, "past")
    assert mask == 0 and not weak[:, :3].any() and torch.equal(weak[:, 3:], cond[:, 3:])
    weak, mask = guidance_conditioning(config, cond, "future")
    assert mask == 1 and not weak[:, 3:].any() and torch.equal(weak[:, :3], cond[:, :3])
    weak, mask = guidance_conditioning(config, cond, "all")
    assert mask == 0 and not weak.any()
    assert torch.equal(cond, keep)
    # the layout is conditioning_fn's: its past block is what "past" zeroes
    from mcvd_pytorch_amd.runner import conditioning_fn
    X = torch.rand(2, 4, 3, 4, 4)
    config.data.image_size = 4
    _, full, _ = conditioning_fn(config, X, num_frames_pred=2)
    torch.manual_seed(0)
    _, dropped, cmask = conditioning_fn(config, X, num_frames_pred=2, prob_mask_cond=1.0)
    weak, mask = guidance_conditioning(config, full, "past")
    assert torch.equal(weak, dropped) and cmask.tolist() == [mask, mask]
