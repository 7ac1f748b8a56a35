"""GPU: the one-piece fp16 Winograd arithmetic -- context option "f16x1", shape ids 24 / 25 (conv_wino2h.cpp with NP = 1).

A DRAFT arithmetic: operands of 11 significant bits.  It is not held to the parity tolerances of tests/test_gpu_parity.py but to
  * per conv, the bound tests/f16x1_ref.py derives (worst case over the signs of the roundings), per element, against an fp64 convolution;
  * per forward and per 100-step sampler run, 3 x the deviation a CPU emulation of the same arithmetic shows (tests/golden/f16x1_drift.pt,
    tools/gen_f16x1_golden.py).  Why 3: the emulation accumulates in fp64 and the kernel in fp32; a few fp16 roundings flip under
    fp32-sized differences of their inputs; the deviation of a sampler run grows like a random walk over its 101 forwards, of which the
    emulation is ONE realisation; an excess beyond that is an arithmetic defect, not rounding.
The option is off by default and authoritative: off means that no one-piece kernel runs, whatever an imported table names.
"""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import synth, unet_ref
from tests import f16x1_ref as R

pytestmark = pytest.mark.gpu

ONE_PIECE = (24, 25)


@pytest.fixture(scope="module")
def ctx():
    from tests.hiputil import Ctx
    return Ctx()


def _net(name):
    from mcvd_pytorch_amd.scorenet import HipScoreNet
    config = synth.make_config(name)
    config.device = "cuda:0"
    sd = synth.make_state_dict(config, seed=123)
    net = HipScoreNet(config)
    missing = net.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return config, sd, net.eval()


def _conv_ops(net):
    """[(op index, ks, kernel that ran, has a norm prologue)] of every conv op of the plan."""
    from mcvd_pytorch_amd import _lib
    n = _lib.lib.mcvd_model_profile_read(net._model, None, None, None, None, None, 0)
    info, out = (C.c_int * 8)(), []
    for i in range(n):
        _lib.check(_lib.lib.mcvd_model_op_info(net._model, i, info), "op_info")
        if info[0] == 3:
            out.append((i, info[2], _lib.lib.mcvd_model_op_kernel(net._model, i), bool(info[7])))
    return n, out


@pytest.fixture(scope="module")
def cfg2(golden_dir):
    """BASELINE config 2 at B = 2 with the reference's fixture and the emulation's: one net for the whole-network tests below (each
    leaves the options as it found them)."""
    g = torch.load(os.path.join(golden_dir, "smmnist_big5_ngf96_b2.pt"), weights_only=False)
    drift = torch.load(os.path.join(golden_dir, "f16x1_drift.pt"), weights_only=False)
    config, sd, net = _net(g["config_name"])
    assert drift["config_name"] == g["config_name"] and drift["batch"] == g["batch"]
    x, cond = synth.make_inputs(config, g["batch"], seed=0)
    noise = synth.make_noise(config, g["batch"], 101, seed=2)
    return dict(g=g, drift=drift, config=config, net=net, x=x.cuda(), cond=cond.cuda(), noise=noise.cuda())


def _sample(c):
    from mcvd_pytorch_amd.samplers import ddpm_sampler
    return ddpm_sampler(c["x"], c["net"], cond=c["cond"], denoise=True, subsample_steps=100, clip_before=True, verbose=False, log=False,
                        noise=c["noise"], final_only=True)[-1:].cpu()


# ------------------------------------------------------------------------------------------------ 1. the option
def test_f16x1_option_exists_and_is_authoritative(cfg2):
    """`f16x1` = 1 is accepted (it was MCVD_EINVAL) and offers the one-piece kernel to the autotuner for 3x3 convs with a NORMALISED input
    only; back at 0 none runs -- after the table tuned with it on was in force, and after that very table is imported again; an imported
    table that names 24 on a raw-input conv runs 10 there even with the option on."""
    from mcvd_pytorch_amd import _lib
    net, x, cond, B = cfg2["net"], cfg2["x"], cfg2["cond"], cfg2["g"]["batch"]
    t = cfg2["g"]["fwd_t"].cuda()
    assert _lib.lib.mcvd_ctx_set_option(net._ctx, b"f16x1", 0) == 0
    b0 = net(x, t, cond=cond).clone()
    _, dflt = _conv_ops(net)
    assert not any(k in ONE_PIECE for _, _, k, _ in dflt), f"one-piece kernels ran by default: {dflt}"
    net.set_option("f16x1", 1)
    a = net(x, t, cond=cond).clone()
    n, on = _conv_ops(net)
    assert any(k in ONE_PIECE for _, _, k, _ in on), f"the f16x1 kernels were offered and never chosen: {on}"
    assert not any(k in ONE_PIECE and (not pro or ks != 3) for _, ks, k, pro in on), f"a raw-input or 1x1 conv ran a one-piece kernel: {on}"
    assert not any(k in (12, 13, 14) for _, _, k, _ in on), f"f16x1 alone switched two-piece kernels on: {on}"
    tuned_on = net.get_tuning(B)
    net.set_option("f16x1", 0)
    b = net(x, t, cond=cond).clone()
    assert not any(k in ONE_PIECE for _, _, k, _ in _conv_ops(net)[1]), "f16x1 = 0 but a one-piece kernel ran"
    assert torch.equal(b, b0) or (b - b0).abs().max().item() <= 2e-5 * b0.abs().max().item()      # (a re-tune may pick other fp32-equivalent kernels)
    assert not torch.equal(a, b)
    net.set_tuning(B, tuned_on)                                   # the table tuned with the option on, installed with it off
    net(x, t, cond=cond)
    ran = _conv_ops(net)[1]
    assert not any(k in ONE_PIECE for _, _, k, _ in ran) and any(k in (10, 11) for _, _, k, _ in ran), ran
    # a table naming 24 on every 3x3 conv, raw-input ones included, with the option ON: the raw ones run 10
    table = [[-1, 0]] * n
    for i, ks, _, _ in on:
        table[i] = [24, 0] if ks == 3 else [15, 1]
    net.set_option("f16x1", 1)
    net.set_tuning(B, table)
    net(x, t, cond=cond)
    ran = _conv_ops(net)[1]
    raw3 = [k for _, ks, k, pro in ran if ks == 3 and not pro]
    print(f"raw-input 3x3 convs under a table naming 24 ran {raw3}")
    # (the stem, a virtual concat whose first part is not a multiple of the chunk, is served by no Winograd kernel: the direct tiles)
    assert 10 in raw3 and all(k == 10 or 0 <= k <= 4 for k in raw3), f"raw-input 3x3 convs under a table naming 24: {raw3}"
    assert all(k == 24 for _, ks, k, pro in ran if ks == 3 and pro), ran
    net.set_option("f16x1", 0)
    net.set_option("bf16x3", 0)                                   # both off: the fp32-MFMA Winograd kernels
    net.set_tuning(B, table)
    net(x, t, cond=cond)
    ran = _conv_ops(net)[1]
    assert all(k in (4, 8) for _, ks, k, pro in ran if ks == 3 and pro) and not any(k >= 10 for _, _, k, _ in ran), ran
    net.set_option("bf16x3", 1)


# ------------------------------------------------------------------------------------------------ 2. the forced kernel against fp64
FORCED = [
    # (shape id, B, C0, C1, Cout, H)
    (24, 3, 48, 0, 32, 8),       # G8 (two images per workgroup, the last one half empty: odd batch), an odd chunk count, COT 1
    (24, 2, 96, 0, 96, 16),      # COT 3
    (24, 1, 64, 32, 64, 32),     # concat input, COT 2, several regions
    (25, 2, 288, 0, 96, 8),      # the K split: partial results + the reduce pass
]


@pytest.mark.parametrize("wscale,xscale", [(1.0, 1.0), (1e-3, 30.0), (40.0, 0.02)], ids=["unit", "small_w_big_x", "big_w_small_x"])
@pytest.mark.parametrize("shape,B,C0,C1,Cout,H", FORCED, ids=lambda v: str(v))
def test_forced_one_piece_kernel_meets_the_derived_bound(ctx, shape, B, C0, C1, Cout, H, wscale, xscale):
    """ids 24 / 25 through the stand-alone conv, every prologue it exposes (raw, affine, affine + SiLU), three magnitude pairs: per
    element, |y - y64| <= the bound of tests/f16x1_ref.py (+ 2^-23 |bias|: the epilogue's two roundings of the bias add, which the bound
    of the bias-free product does not know).  Bit-identical run to run, and not what the two-piece kernel (12 / 13) computes."""
    from mcvd_pytorch_amd import _lib
    g = torch.Generator().manual_seed(31)
    Cin = C0 + C1
    x = torch.randn(B, Cin, H, H, generator=g) * xscale
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5 * wscale
    bias = 0.1 * torch.randn(Cout, generator=g) * wscale * xscale
    coef = torch.stack([(1 + 0.3 * torch.randn(B, Cin, generator=g)), 0.3 * xscale * torch.randn(B, Cin, generator=g)], -1).contiguous()
    x0, x1 = (x[:, :C0].contiguous().cuda(), x[:, C0:].contiguous().cuda()) if C1 else (x.cuda(), None)
    worst = 0.0
    for pro in (0, 1, 2):
        kw = dict(x1=x1, coef=coef.cuda() if pro else None, act=1 if pro == 2 else 0)
        ctx.opt("conv_shape", shape)
        got = ctx.conv2d(x0, w.cuda(), bias.cuda(), **kw)
        assert _lib.lib.mcvd_last_conv_kernel() == shape, (shape, _lib.lib.mcvd_last_conv_kernel())
        again = ctx.conv2d(x0, w.cuda(), bias.cuda(), **kw)
        ctx.opt("conv_shape", shape - 12)
        two = ctx.conv2d(x0, w.cuda(), bias.cuda(), **kw)
        assert _lib.lib.mcvd_last_conv_kernel() == shape - 12
        ctx.opt("conv_shape", -1)
        d = R.activate(x, coef if pro else None, pro == 2)
        y64 = F.conv2d(d, w.double(), bias.double(), padding=1)
        _, bound = R.wino_f16x1(d, w)
        bound = bound + 2.0 ** -23 * bias.double().abs().reshape(1, -1, 1, 1)
        err = (got.cpu().double() - y64).abs()
        ratio = (err / bound).max().item()
        worst = max(worst, ratio)
        print(f"f16x1 id {shape} B{B} {C0}+{C1}->{Cout} @{H} w*{wscale} x*{xscale} pro {pro}: worst |err| / bound {ratio:.4f}, "
              f"max|err| / max|y| {err.max().item() / y64.abs().max().item():.2e}")
        assert torch.isfinite(got).all()
        assert (err <= bound).all(), f"pro {pro}: |err| / bound = {ratio:.3f}"
        assert torch.equal(got, again), f"pro {pro}: two runs differ"
        assert not torch.equal(got, two), f"pro {pro}: bit-equal to the two-piece kernel's output"
        assert err.max().item() > 1e-5 * y64.abs().max().item(), "fp32-sized error: one fp16 piece did not run"
    print(f"f16x1 id {shape} worst ratio over the prologues: {worst:.4f}")


# ------------------------------------------------------------------------------------------------ 3. the range guard
def test_f16x1_overflow_is_reported_and_the_default_path_has_the_range():
    """The net of test_f16x2_overflow_is_reported_and_the_default_path_has_the_range (temb projections scaled by 3e4: finite GroupNorm-ed
    activations of ~5e4, beyond 65504 / 64 in the transform domain) with ONLY f16x1 on: the default path reproduces the oracle, the
    one-piece kernel's Inf -> NaN is reported as MCVD_ERANGE naming the option that is on, by the context and by both sampler loops."""
    from mcvd_pytorch_amd import _lib
    from mcvd_pytorch_amd.samplers import ddpm_sampler
    from mcvd_pytorch_amd.scorenet import HipScoreNet
    config = synth.make_config("tiny")
    config.device = "cuda:0"
    sd = synth.make_state_dict(config, seed=123)
    for k in sd:
        if "Dense_0.weight" in k:
            sd[k] = sd[k] * 3.0e4
    net = HipScoreNet(config)
    net.load_state_dict(sd, strict=True)
    net.eval()
    x, cond = synth.make_inputs(config, 2, seed=0)
    t = torch.tensor([990, 130])
    with torch.no_grad():
        ref = unet_ref.unet_forward(sd, config, x, t, cond)
    assert torch.isfinite(ref).all()
    eps = net(x.cuda(), t.cuda(), cond=cond.cuda()).cpu()
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


# ------------------------------------------------------------------------------------------------ 4. one forward
def test_forward_under_f16x1_is_within_three_times_the_emulation(cfg2):
    net, g, drift = cfg2["net"], cfg2["g"], cfg2["drift"]
    net.set_option("f16x1", 1)
    eps = net(cfg2["x"], g["fwd_t"].cuda(), cond=cfg2["cond"]).cpu()
    ran = _conv_ops(net)[1]
    net.set_option("f16x1", 0)
    d = (eps - g["fwd_eps"]).abs()
    print(f"f16x1 forward: max-abs {d.max().item():.3e} ({d.max().item() / drift['fwd_max_abs']:.2f} x emulated), mean-abs {d.mean().item():.3e} "
          f"({d.mean().item() / drift['fwd_mean_abs']:.2f} x emulated); {sum(k in ONE_PIECE for _, _, k, _ in ran)} convs on the one-piece kernel")
    assert any(k in ONE_PIECE for _, _, k, _ in ran)
    assert d.max().item() <= 3 * drift["fwd_max_abs"] and d.mean().item() <= 3 * drift["fwd_mean_abs"]


# ------------------------------------------------------------------------------------------------ 5. / 6. the sampler
@pytest.mark.parametrize("with_f16x2", [0, 1], ids=["f16x1", "f16x1+f16x2"])
def test_sampler_under_f16x1_is_within_three_times_the_emulation(cfg2, with_f16x2):
    """ddpm_sampler, 100 steps + denoise, injected noise, against the reference's frames: max-abs and mean-abs within 3 x the emulation's
    (module docstring); different from the default arithmetic's frames; and the default arithmetic, in the same process after the options
    are switched back, still meets its unchanged 1e-4: nothing leaks."""
    net, g, drift = cfg2["net"], cfg2["g"], cfg2["drift"]
    ref = g["sampler_ddpm_100"]["result"]
    net.set_option("f16x1", 1)
    net.set_option("f16x2", with_f16x2)
    out = _sample(cfg2)
    ran = _conv_ops(net)[1]
    net.set_option("f16x1", 0)
    net.set_option("f16x2", 0)
    dflt = _sample(cfg2)
    assert out.shape == ref.shape and torch.isfinite(out).all()
    d = (out - ref).abs()
    print(f"f16x1{' + f16x2' if with_f16x2 else ''} DDPM-100: max-abs {d.max().item():.3e} ({d.max().item() / drift['sampler_max_abs']:.2f} x emulated "
          f"{drift['sampler_max_abs']:.3e}), mean-abs {d.mean().item():.3e} ({d.mean().item() / drift['sampler_mean_abs']:.2f} x emulated "
          f"{drift['sampler_mean_abs']:.3e}); {sum(k in ONE_PIECE for _, _, k, _ in ran)} convs on the one-piece kernel")
    assert any(k in ONE_PIECE for _, _, k, _ in ran)
    assert d.max().item() <= 3 * drift["sampler_max_abs"] and d.mean().item() <= 3 * drift["sampler_mean_abs"]
    assert not torch.equal(out, dflt)
    assert not any(k in ONE_PIECE + (12, 13, 14) for _, _, k, _ in _conv_ops(net)[1])
    assert (dflt - ref).abs().max().item() <= 1e-4, "the default arithmetic after f16x1 was switched off again"
