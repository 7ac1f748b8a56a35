"""CPU: the caller-side glue restated in mcvd_pytorch_amd/runner.py (conditioning layout, data transforms)."""
import torch

from oracle import synth


def _runner():
    from mcvd_pytorch_amd import runner
    return runner


def test_conditioning_fn_layout_is_frame_major():
    """runners/ncsn_runner.py:115-118: channel index = t*C + c; cond = [past..., future...]."""
    r = _runner()
    cfg = synth.make_config("tiny_spade")           # C=3, nf=2, past=1, future=1
    d = cfg.data
    B, C, S = 2, d.channels, d.image_size
    T = d.num_frames_cond + d.num_frames + d.num_frames_future
    X = torch.arange(B * T * C).float().reshape(B, T, C, 1, 1).expand(B, T, C, S, S).contiguous()
    pred, cond, mask = r.conditioning_fn(cfg, X, num_frames_pred=d.num_frames)
    assert mask is None
    assert pred.shape == (B, C * d.num_frames, S, S) and cond.shape == (B, C * (d.num_frames_cond + d.num_frames_future), S, S)
    for t in range(d.num_frames):
        for c in range(C):
            assert torch.equal(pred[:, t * C + c], X[:, d.num_frames_cond + t, c])
    assert torch.equal(cond[:, :C], X[:, 0])                                    # past frame
    assert torch.equal(cond[:, C:2 * C], X[:, d.num_frames_cond + d.num_frames])  # future frame
    _, cond0, _ = r.conditioning_fn(cfg, X, num_frames_pred=d.num_frames, prob_mask_future=1.0)
    assert cond0[:, C:].abs().max() == 0                                        # :130-131 all-zero future block


def test_conditioning_masks_zero_whole_samples_and_keep_the_draw_order():
    """prob_mask_cond / prob_mask_future (runners/ncsn_runner.py:119-145): per-sample keep masks, cond mask drawn before the future
    mask, int32 cond_mask returned, `prob_mask_sync` reuses the cond mask for the future block."""
    r = _runner()
    cfg = synth.make_config("tiny_spade")           # past = 1, future = 1
    d = cfg.data
    B, C, S = 64, d.channels, d.image_size
    T = d.num_frames_cond + d.num_frames + d.num_frames_future
    X = 1.0 + torch.rand(B, T, C, S, S)
    torch.manual_seed(5)
    pred, cond, mask = r.conditioning_fn(cfg, X, num_frames_pred=d.num_frames, prob_mask_cond=0.5, prob_mask_future=0.5)
    torch.manual_seed(5)
    m1 = torch.rand(B) > 0.5
    m2 = torch.rand(B) > 0.5
    assert mask.dtype == torch.int32 and torch.equal(mask.bool(), m1)
    past, fut = cond[:, :C], cond[:, C:]
    assert torch.equal(past.flatten(1).abs().sum(1) > 0, m1) and torch.equal(fut.flatten(1).abs().sum(1) > 0, m2)
    assert torch.equal(pred, X[:, d.num_frames_cond:d.num_frames_cond + d.num_frames].flatten(1, 2))
    d.prob_mask_sync = True
    torch.manual_seed(5)
    _, cond_s, mask_s = r.conditioning_fn(cfg, X, num_frames_pred=d.num_frames, prob_mask_cond=0.5, prob_mask_future=0.5)
    assert torch.equal(cond_s[:, C:].flatten(1).abs().sum(1) > 0, mask_s.bool())
    d.prob_mask_sync = False
    flat, none_c, none_m = r.conditioning_fn(cfg, X, conditional=False)
    assert none_c is None and none_m is None and torch.equal(flat, X.flatten(1, 2))


def test_data_transform_switches():
    """uniform dequantisation stays inside [0, 1), the logit transform inverts through the sigmoid, a mean image is removed and
    restored (datasets/__init__.py:235-261)."""
    r = _runner()
    cfg = synth.make_config("tiny")
    d = cfg.data
    X = torch.rand(2, 4, 1, 8, 8)
    d.rescaled, d.logit_transform = False, True
    Y = r.data_transform(cfg, X)
    lam = 1e-6
    Xl = lam + (1 - 2 * lam) * X
    assert torch.equal(Y, torch.log(Xl) - torch.log1p(-Xl))
    assert torch.allclose(r.inverse_data_transform(cfg, Y), Xl, atol=1e-6)
    d.logit_transform, d.rescaled, d.uniform_dequantization = False, False, True
    Y = r.data_transform(cfg, X)
    assert (Y >= X / 256. * 255.).all() and (Y < X / 256. * 255. + 1 / 256. + 1e-7).all()
    d.uniform_dequantization, d.rescaled = False, True
    cfg.image_mean = torch.full((4, 1, 8, 8), 0.25)
    Y = r.data_transform(cfg, X)
    assert torch.allclose(Y, 2 * X - 1 - 0.25) and torch.allclose(r.inverse_data_transform(cfg, Y), X, atol=1e-6)
    del cfg.image_mean


def test_data_transform_round_trip():
    r = _runner()
    cfg = synth.make_config("tiny")
    X = torch.rand(2, 4, 1, 8, 8)
    Y = r.data_transform(cfg, X)
    assert Y.min() >= -1 and Y.max() <= 1 and torch.allclose(Y, 2 * X - 1)
    assert torch.allclose(r.inverse_data_transform(cfg, Y), X, atol=1e-6)
    assert r.inverse_data_transform(cfg, Y * 3).max() <= 1.0                    # clamp (datasets/__init__.py:261)


def test_save_video_pred_format(tmp_path):
    """videos_pred_<ckpt>.pt: a dict of CPU tensors with the reference's keys (ncsn_runner.py:2106-2112)."""
    r = _runner()
    cond, pred, real = torch.rand(2, 4, 8, 8), torch.rand(2, 6, 8, 8), torch.rand(2, 6, 8, 8)
    p = r.save_video_pred(str(tmp_path / "videos_pred_1000.pt"), cond, pred, real)
    d = torch.load(p, weights_only=False)
    assert sorted(d) == ["cond", "pred", "real"] and torch.equal(d["pred"], pred) and d["cond"].device.type == "cpu"


# ------------------------------------------------------------------ round 6: fixtures from the REAL NCSNRunner.video_gen
RUNNER_FIXTURES = ["tiny_runner_videogen.pt",               # prediction, three blocks of two frames cropped to five
                   "tiny_runner_videogen_prevt.pt",         # sampling.init_prev_t = 0.5: blocks restart from the previous block's frames, re-noised
                   "tiny_runner_videogen_oneframe.pt",      # sampling.one_frame_at_a_time: cond shifts by one frame per block
                   "tiny_runner_videogen_plain.pt",         # sampling.denoise = False, clip_before = False: the switches the loop forwards (|frames| reach 1e3)
                   "tiny_runner_videogen_ddim.pt",          # model.version = "DDIM": NCSNRunner.get_sampler binds ddim_sampler (:2702-2714), the same block loop
                   "tiny_runner_videogen_fpndm.pt"]         # model.version = "FPNDM"


def _runner_tol(g):
    """1e-4 on [-1, 1] frames; where clip_before = False lets them reach 1e3, 1e-5 of their range (the fixtures' surface cases use the same rule).
    The deterministic samplers (DDIM, F-PNDM) neither clip the last iterate nor inject noise: their three-block chains amplify fp32 rounding
    (the reference's own fp32 chain is 2.7e-3 / 1.2e-3 from its fp64 restatement, recorded in the fixture) -- the gate is 3 x that drift, as for
    the DDIM sampler fixtures; a wrong cond shift or crop is an O(1) error."""
    if g.get("version", "DDPM") != "DDPM":
        return 3.0 * g["ref32_vs_ref64_max_abs"]
    return 1e-4 if g.get("overrides", {}).get("clip_before", True) else 1e-5 * float(g["pred_raw"].abs().max())


def _runner_fixture(golden_dir, name="tiny_runner_videogen.pt"):
    from tests.golden_io import load_golden
    return load_golden(golden_dir, name)


def _runner_config(g):
    cfg = synth.make_config(g["config_name"])
    cfg.sampling.num_frames_pred, cfg.sampling.subsample = g["nfp"], g["subsample"]
    cfg.model.version = g.get("version", "DDPM")
    for k, v in g.get("overrides", {}).items():
        setattr(cfg.sampling, k, v)
    return cfg


import pytest  # noqa: E402


@pytest.mark.parametrize("fx", RUNNER_FIXTURES)
def test_glue_matches_the_real_runner(golden_dir, fx):
    """data_transform / conditioning_fn / inverse_data_transform of mcvd_pytorch_amd.runner against what the REAL
    `runners.ncsn_runner.NCSNRunner.video_gen` computed on the same clips (oracle/gen_runner_golden.py: the real module, imported with
    stand-ins for the absent third-party packages, driven through :1304-1570): bit for bit -- these are pure index / affine maps."""
    r = _runner()
    g = _runner_fixture(golden_dir, fx)
    cfg = _runner_config(g)
    batch = g["clips"][g["order"]]                                       # the rows the shuffling DataLoader served
    real_t = r.data_transform(cfg, batch)
    assert torch.equal(real_t, g["real_t"])
    real, cond, mask = r.conditioning_fn(cfg, real_t, num_frames_pred=g["nfp"], prob_mask_cond=0.0, prob_mask_future=0.0, conditional=True)
    assert mask is None and g["cond_mask"] is None
    assert torch.equal(real, g["real"]) and torch.equal(cond, g["cond"])
    assert torch.equal(r.inverse_data_transform(cfg, real), g["real01"])
    assert torch.equal(r.inverse_data_transform(cfg, cond.clone()), g["cond01"])
    assert torch.equal(r.inverse_data_transform(cfg, g["pred_raw"]), g["pred01"])
    # what the runner hands the sampler (:1513-1520): exactly the kwargs the mirror's block loop passes on
    kw = g["sampler_kwargs"][0]
    ov = g.get("overrides", {})
    assert kw == dict(cond_mask=None, n_steps_each=0, step_lr=0.0, verbose=True, final_only=True, denoise=ov.get("denoise", True),
                      subsample_steps=g["subsample"], clip_before=ov.get("clip_before", True), t_min=float(ov.get("init_prev_t", -1.0)), log=True,
                      gamma=False)


@pytest.mark.parametrize("fx", RUNNER_FIXTURES)
def test_block_loop_matches_the_real_runner(golden_dir, fx):
    """The mirror's autoregressive block loop (runner.video_gen) around the CPU oracle net and the oracle sampler, fed the REAL runner's
    block inits and step noise: the frames `NCSNRunner.video_gen` had assembled at :1569 (3 blocks of 2 frames cropped to 5: cond shift
    :1532-1535, crop :1569)."""
    from oracle import sampler_ref, unet_ref
    r = _runner()
    g = _runner_fixture(golden_dir, fx)
    cfg = _runner_config(g)
    t_min = float(g.get("overrides", {}).get("init_prev_t", -1.0))
    net = unet_ref.OracleScoreNet(cfg, synth.make_state_dict(cfg, seed=123))
    net.device = torch.device("cpu")
    blk = [0]

    def sampler(x, scorenet, cond=None, **kw):
        b = blk[0]
        blk[0] += 1
        k = [0]

        def fn(i, like):
            k[0] += 1
            return g["step_noise"][b, k[0] - 1]
        ov = g.get("overrides", {})
        assert kw["final_only"] and kw["subsample_steps"] == g["subsample"] and kw["t_min"] == t_min
        assert kw["denoise"] == ov.get("denoise", True) and kw["clip_before"] == ov.get("clip_before", True)      # the config switches reach the sampler
        version = g.get("version", "DDPM")
        if version == "FPNDM":
            return sampler_ref.fpndm_sample(x, scorenet, cond=cond, final_only=True, subsample_steps=kw["subsample_steps"], clip_before=kw["clip_before"])
        return sampler_ref.sample(x, scorenet, cond=cond, kind=version.lower(), final_only=True, denoise=kw["denoise"], subsample_steps=kw["subsample_steps"],
                                  clip_before=kw["clip_before"], t_min=kw["t_min"], noise_fn=fn)
    pred = r.video_gen(cfg, net, g["cond"], num_frames_pred=g["nfp"], sampler=sampler, init_noise_fn=lambda i, shp, dev: g["z_init"][i])
    assert blk[0] == 3 and pred.shape == g["pred_raw"].shape
    tol = _runner_tol(g)
    assert 0.0 < g["ref32_vs_ref64_max_abs"] <= tol / 3 * (1 + 1e-6)
    err = (pred - g["pred_raw"]).abs().max().item()
    assert err <= tol, f"block loop vs the real runner: {err:.3e} (gate {tol:.1e})"
