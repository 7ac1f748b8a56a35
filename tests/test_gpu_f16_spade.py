"""GPU: the fp16 arithmetics (context options "f16x2", "f16x1") on SPADE nets.

A 3x3 conv behind a SPADE norm reads the tensor spade_apply materialises -- silu(((A x + B)(1 + gamma) + beta) s1 + b2): a normalised,
modulated, activated value -- and counts as a conv with a NORMALISED input: the autotuner offers it the two-piece (12 / 13 / 26) and
one-piece (24 / 25 / 27) Winograd kernels, and an imported table that names them keeps them there.  The stem, the shortcuts, the convs
behind a FIR resampler and the cond-only SPADE prep convs (mlp_shared / mlp_gamma / mlp_beta) read raw tensors and stay on the
fp32-range kernels; with spade_fuse = 1 the modulation stays in the fp32 Winograd loader and no fp16 kernel reaches those convs.

Gates: f16x2 claims fp32-equivalent results -- the 1e-4 gates of tests/test_gpu_parity.py against the REAL reference's fixtures of BASELINE
config 4 (bair_big_spade, B = 2); f16x1 is a draft arithmetic -- 3 x the deviation a CPU emulation of it shows (tests/golden/
f16x1_spade_drift.pt, tools/gen_f16x1_spade_golden.py; the rule and its reason: tests/test_gpu_f16x1.py).  Beyond the fp16 range -- here a
cond-derived gamma of thousands -- the kernels give NaN and the library says MCVD_ERANGE, naming the option.
"""
import ctypes as C
import os

import pytest
import torch

from oracle import synth, unet_ref

pytestmark = pytest.mark.gpu

TWO_PIECE = (12, 13, 26)
ONE_PIECE = (24, 25, 27)


def _net(name, sd=None):
    from mcvd_pytorch_amd.scorenet import HipScoreNet
    config = synth.make_config(name)
    config.device = "cuda:0"
    sd = sd if sd is not None else synth.make_state_dict(config, seed=123)
    net = HipScoreNet(config)
    missing = net.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return config, sd, net.eval()


def _conv_ops(net):
    """[(op index, ks, kernel that ran, has a norm in front, module)] of every conv op of the plan.  In a SPADE net every norm in front of a
    conv is a SPADE norm; the prep convs have module -1 and no norm; the stem, the shortcuts and the convs behind a FIR have no norm."""
    from mcvd_pytorch_amd import _lib
    n = _lib.lib.mcvd_model_profile_read(net._model, None, None, None, None, None, 0)
    info, out = (C.c_int * 8)(), []
    for i in range(n):
        _lib.check(_lib.lib.mcvd_model_op_info(net._model, i, info), "op_info")
        if info[0] == 3:
            out.append((i, info[2], _lib.lib.mcvd_model_op_kernel(net._model, i), bool(info[7]), info[1]))
    return n, out


def _spade3(ran):
    return [k for _, ks, k, pro, mod in ran if ks == 3 and pro and mod >= 0]


def _others(ran):
    return [(ks, k, mod) for _, ks, k, pro, mod in ran if not (ks == 3 and pro and mod >= 0)]


@pytest.fixture(scope="module")
def cfg4(golden_dir):
    """BASELINE config 4 at B = 2: the reference's fixtures, the emulation's, the oracle's eps (the forward fixture holds a strided probe
    only), one net for the whole-network tests below (each leaves the options as it found them)."""
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    gf = torch.load(os.path.join(golden_dir, "bair_big_spade_b2_fwd.pt"), weights_only=False)
    gs = torch.load(os.path.join(golden_dir, "bair_big_spade_b2_ddpm100.pt"), weights_only=False)
    drift = torch.load(os.path.join(golden_dir, "f16x1_spade_drift.pt"), weights_only=False)
    assert drift["config_name"] == gf["config_name"] == gs["config_name"] and drift["batch"] == gf["batch"] == gs["batch"] == 2
    assert drift["steps"] == gs["subsample"] == 100 and drift["fwd_reference"] == "oracle"
    config, sd, net = _net(gf["config_name"])
    x, cond = synth.make_inputs(config, 2, seed=0)
    noise = synth.make_noise(config, 2, 101, seed=2)
    with torch.no_grad():
        ref = unet_ref.unet_forward(sd, config, x, gf["fwd_t"], cond)
    return dict(gf=gf, gs=gs, drift=drift, config=config, net=net, x=x.cuda(), cond=cond.cuda(), noise=noise.cuda(), ref=ref, t=gf["fwd_t"].cuda())


def _fwd(c):
    """One forward; the cond tensor is a fresh copy, so the cond-only prep convs run (and are recorded) under the options in force."""
    return c["net"](c["x"], c["t"], cond=c["cond"].clone()).clone()


def _sample(c):
    from mcvd_pytorch_amd.samplers import ddpm_sampler
    return ddpm_sampler(c["x"], c["net"], cond=c["cond"].clone(), denoise=True, subsample_steps=100, clip_before=True, verbose=False, log=False,
                        noise=c["noise"], final_only=True)[-1:].cpu()


# ------------------------------------------------------------------------------------------------ 1. which convs the options reach
def test_options_reach_the_convs_behind_spade_norms_and_no_others(cfg4):
    net, B = cfg4["net"], 2
    b0 = _fwd(cfg4)
    table0 = net.get_tuning(B)
    _, dflt = _conv_ops(net)
    assert not any(k in TWO_PIECE + ONE_PIECE + (14,) for _, _, k, _, _ in dflt), f"fp16 kernels ran by default: {dflt}"
    assert len(_spade3(dflt)) >= 40 and any(mod < 0 for _, _, _, _, mod in dflt), "the classification found no SPADE / prep convs"
    tuned = {}
    for opt, ids in (("f16x2", TWO_PIECE), ("f16x1", ONE_PIECE)):
        net.set_option(opt, 1)
        a = _fwd(cfg4)
        _, on = _conv_ops(net)
        tuned[opt] = net.get_tuning(B)
        net.set_option(opt, 0)
        s3 = _spade3(on)
        print(f"{opt}: 3x3 convs behind SPADE norms ran {sorted((k, s3.count(k)) for k in set(s3))}; the others {sorted(set(_others(on)))}")
        assert any(k in ids for k in s3), f"{opt} = 1: no conv behind a SPADE norm ran one of {ids}: {s3}"
        wrong = [o for o in _others(on) if o[1] in ONE_PIECE + TWO_PIECE]
        assert not wrong, f"{opt} = 1: a prep conv, the stem, a shortcut or a 1x1 (ks, kernel, module) ran an fp16 Winograd id: {wrong}"
        assert not any(k in ONE_PIECE for _, _, k, _, _ in on) or opt == "f16x1"
        assert not torch.equal(a, b0)
    b = _fwd(cfg4)                                               # both options back at 0 (the table was re-tuned in between)
    _, off = _conv_ops(net)
    assert not any(k in TWO_PIECE + ONE_PIECE + (14,) for _, _, k, _, _ in off), f"options off but these ran: {off}"
    assert torch.equal(b, b0) or (b - b0).abs().max().item() <= 2e-5 * b0.abs().max().item()
    for opt in tuned:                                            # the tables tuned with an option on, imported with it off: the options win
        named = [sh for sh, _ in tuned[opt]]
        net.set_tuning(B, tuned[opt])
        _fwd(cfg4)
        _, imp = _conv_ops(net)
        assert not any(k in TWO_PIECE + ONE_PIECE + (14,) for _, _, k, _, _ in imp), f"table of {opt} = 1 imported with the option off: {imp}"
        k4 = [k for i, _, k, _, _ in imp if named[i] in (26, 27)]
        print(f"{opt}: the {len(k4)} ops its table has on 26 / 27 ran {sorted(set(k4))} with the option off")
        assert all(k == 18 for k in k4), k4
    net.set_tuning(B, table0)                                    # ... and under the first run's own table: the same bits
    assert torch.equal(_fwd(cfg4), b0), "options off, the first run's table installed: eps is not bit-identical to the first run"
    # spade_fuse = 1: the modulation stays in the fp32 Winograd loader, the fp16 options do not reach those convs
    net.set_option("spade_fuse", 1)
    net.set_option("f16x2", 1)
    net.set_option("f16x1", 1)
    try:
        f = _fwd(cfg4)
        _, fused = _conv_ops(net)
    finally:
        net.set_option("f16x2", 0)
        net.set_option("f16x1", 0)
        net.set_option("spade_fuse", 0)
    assert not any(k in TWO_PIECE + ONE_PIECE for k in _spade3(fused)), f"spade_fuse = 1: SPADE convs on fp16 kernels: {_spade3(fused)}"
    assert (f.cpu() - cfg4["ref"]).abs().max().item() <= 1e-4 * cfg4["ref"].abs().max().item()


def test_imported_table_naming_24_runs_it_behind_spade_norms_only():
    """tiny_spade, B = 2, a table naming 24 on every 3x3 conv: with f16x1 on the convs behind SPADE norms run 24, the prep convs, the stem
    and the convs behind a FIR (raw inputs) run 10 or a direct tile; with the option off every conv behind a SPADE norm runs 10 / 11 and the
    raw-input ones what they ran before."""
    config, sd, net = _net("tiny_spade")
    x, cond = synth.make_inputs(config, 2, seed=0)
    t = torch.tensor([700, 20]).cuda()
    net(x.cuda(), t, cond=cond.cuda())
    n, ops = _conv_ops(net)
    table = [[-1, 0]] * n
    for i, ks, _, _, _ in ops:
        if ks == 3:
            table[i] = [24, 0]
    net.set_option("f16x1", 1)
    net.set_tuning(2, table)
    a = net(x.cuda(), t, cond=cond.clone().cuda()).cpu()
    ran = _conv_ops(net)[1]
    s3 = _spade3(ran)
    raw3 = [k for ks, k, _ in _others(ran) if ks == 3]
    print(f"table naming 24, f16x1 on: behind SPADE norms {s3}; raw-input 3x3 convs {raw3}")
    assert s3 and all(k == 24 for k in s3), s3
    assert raw3 and all(k == 10 or 0 <= k <= 4 for k in raw3), raw3
    assert any(mod < 0 and ks == 3 for _, ks, _, _, mod in ran)
    net.set_option("f16x1", 0)
    net.set_tuning(2, table)
    b = net(x.cuda(), t, cond=cond.clone().cuda()).cpu()
    ran = _conv_ops(net)[1]
    k3 = [k for _, ks, k, _, _ in ran if ks == 3]
    print(f"the same table, f16x1 off: {k3}")
    # every conv the three-piece kernel serves runs it: all of those behind SPADE norms; the raw-input ones run what they ran with the option
    # on (10, or a direct tile where no Winograd kernel takes the layer: mlp_shared over the cond frames, the stem)
    assert all(k in (10, 11) for k in _spade3(ran)), _spade3(ran)
    assert [k for ks, k, _ in _others(ran) if ks == 3] == raw3 and 10 in raw3
    assert not any(k in ONE_PIECE + TWO_PIECE for k in k3)
    with torch.no_grad():
        ref = unet_ref.unet_forward(sd, config, x, t.cpu(), cond)
    assert (b - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()
    assert not torch.equal(a, b) and torch.isfinite(a).all()


# ------------------------------------------------------------------------------------------------ 2. f16x2: parity
def test_config4_under_f16x2_meets_the_parity_gates(cfg4):
    """eps against the reference's probe and the oracle, the 100-step DDPM frames against the reference's: 1e-4, as under the default."""
    net, gf, gs = cfg4["net"], cfg4["gf"], cfg4["gs"]
    net.set_option("f16x2", 1)
    try:
        eps = _fwd(cfg4).cpu()
        s3 = _spade3(_conv_ops(net)[1])
        out = _sample(cfg4)
    finally:
        net.set_option("f16x2", 0)
    assert any(k in TWO_PIECE for k in s3), s3
    p, ref = gf["fwd_eps_probe"], cfg4["ref"]
    assert list(eps.shape) == p["shape"]
    e_probe = (eps.reshape(-1).double()[p["idx"]].float() - p["sample"]).abs().max().item()
    e_ref = (eps - ref).abs().max().item()
    e_out = (out - gs["result"]).abs().max().item()
    print(f"config 4 under f16x2 ({sum(k in TWO_PIECE for k in s3)} of {len(s3)} SPADE convs two-piece): eps vs probe {e_probe:.3e}, vs oracle {e_ref:.3e} "
          f"(max|eps| {ref.abs().max().item():.3f}); DDPM-100 frames {e_out:.3e}")
    assert e_probe <= 1e-4 * p["sample"].abs().max().item()
    assert e_ref <= 1e-4 * ref.abs().max().item()
    assert out.shape == gs["result"].shape and e_out <= 1e-4


# ------------------------------------------------------------------------------------------------ 3. f16x1: drift
def test_config4_under_f16x1_is_within_three_times_the_emulation(cfg4):
    net, gs, drift, ref = cfg4["net"], cfg4["gs"], cfg4["drift"], cfg4["ref"]
    net.set_option("f16x1", 1)
    try:
        eps = _fwd(cfg4).cpu()
        s3 = _spade3(_conv_ops(net)[1])
        out = _sample(cfg4)
    finally:
        net.set_option("f16x1", 0)
    assert any(k in ONE_PIECE for k in s3), s3
    df, ds = (eps - ref).abs(), (out - gs["result"]).abs()
    print(f"config 4 under f16x1 ({sum(k in ONE_PIECE for k in s3)} of {len(s3)} SPADE convs one-piece; {drift['convs_per_forward']} emulated): forward max-abs "
          f"{df.max().item():.3e} ({df.max().item() / drift['fwd_max_abs']:.2f} x emulated), mean-abs {df.mean().item():.3e} "
          f"({df.mean().item() / drift['fwd_mean_abs']:.2f} x); DDPM-100 max-abs {ds.max().item():.3e} ({ds.max().item() / drift['sampler_max_abs']:.2f} x "
          f"emulated {drift['sampler_max_abs']:.3e}), mean-abs {ds.mean().item():.3e} ({ds.mean().item() / drift['sampler_mean_abs']:.2f} x)")
    assert torch.isfinite(out).all() and out.shape == gs["result"].shape
    assert df.max().item() <= 3 * drift["fwd_max_abs"] and df.mean().item() <= 3 * drift["fwd_mean_abs"]
    assert ds.max().item() <= 3 * drift["sampler_max_abs"] and ds.mean().item() <= 3 * drift["sampler_mean_abs"]
    assert df.max().item() > 1e-4 * ref.abs().max().item(), "fp32-sized deviation: no one-piece kernel took part"


# ------------------------------------------------------------------------------------------------ 4. the range guard behind a SPADE norm
GAMMA_SCALE = 1000.0      # mlp_gamma weights of tiny_spade times this: on the CPU the oracle stays finite (max|eps| 1.6e3), the largest materialised
                          # value is 6.9e3 -- beyond 65504 / 64 = 1023.5 -- and the emulation of tests/f16x1_ref.py on those convs gives Inf / NaN


def test_overflow_behind_a_spade_norm_is_reported_and_the_default_path_has_the_range():
    from mcvd_pytorch_amd import _lib
    from mcvd_pytorch_amd.samplers import ddpm_sampler
    config = synth.make_config("tiny_spade")
    sd = synth.make_state_dict(config, seed=123)
    for k in sd:
        if "mlp_gamma.weight" in k:
            sd[k] = sd[k] * GAMMA_SCALE
    config, sd, net = _net("tiny_spade", sd)
    x, cond = synth.make_inputs(config, 2, seed=0)
    t = torch.tensor([990, 130])
    seen, orig = [0.0], unet_ref.act_norm

    def watched(*a):
        o = orig(*a)
        seen[0] = max(seen[0], float(o.abs().max()))
        return o
    unet_ref.act_norm = watched
    try:
        with torch.no_grad():
            ref = unet_ref.unet_forward(sd, config, x, t, cond)
    finally:
        unet_ref.act_norm = orig
    assert torch.isfinite(ref).all() and seen[0] > 65504 / 64, seen
    eps = net(x.cuda(), t.cuda(), cond=cond.cuda()).cpu()
    print(f"gamma x {GAMMA_SCALE}: largest materialised value {seen[0]:.4g}, max|eps| {ref.abs().max().item():.4g}, default path off by "
          f"{(eps - ref).abs().max().item():.3e}")
    assert (eps - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()
    assert _lib.lib.mcvd_ctx_check_range(net._ctx) == 0
    net.set_option("f16x1", 1)
    net.set_option("conv_shape", 24)
    bad = net(x.cuda(), t.cuda(), cond=cond.cuda()).cpu()
    assert not torch.isfinite(bad).all()
    assert _lib.lib.mcvd_ctx_check_range(net._ctx) == -5
    msg = _lib.lib.mcvd_last_error(None)
    assert b"f16x1" in msg and b"f16x2" not in msg, msg
    assert _lib.lib.mcvd_ctx_check_range(net._ctx) == 0                     # the record is cleared by the call
    for fo in (True, False):                                                # device loop and host loop
        with pytest.raises(RuntimeError, match="f16x1"):
            ddpm_sampler(x.cuda(), net, cond=cond.cuda(), final_only=fo, subsample_steps=5, seed=1)
    net.set_option("f16x1", 0)                                              # switching the option clears a stale verdict
    net.set_option("conv_shape", -1)
    eps = net(x.cuda(), t.cuda(), cond=cond.cuda()).cpu()
    assert (eps - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() and _lib.lib.mcvd_ctx_check_range(net._ctx) == 0
