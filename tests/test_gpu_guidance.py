"""GPU: classifier-free guidance in the samplers (include/mcvd_hip.h "classifier-free guidance", samplers.py, runner.py).

Semantics under test: w = float32(s - 1); per element d = e_c - e_u, e = e_c + w d, one fp32 rounding per operation, no fma; e_c on
(x, cond), e_u on (x, cond_weak) -- rows [0, B) and [B, 2B) of ONE forward at 2B rows; noise belongs to the B rows of the call.
Everything but the fixture comparison (test 5) is bit for bit."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from oracle import synth
from tests.golden_io import load_golden

pytestmark = pytest.mark.gpu

DDPM, DDIM = 0, 1
SCALES = (1.0, 0.0, 2.5, -0.5)
BIG = 8192 * 1024 + 28          # float4 count above one trip of the 8192 x 256 grid-stride loop


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _net(name):
    from mcvd_pytorch_amd.scorenet import HipScoreNet
    config = synth.make_config(name)
    config.device = "cuda:0"
    net = HipScoreNet(config)
    net.load_state_dict(synth.make_state_dict(config, seed=123), strict=True)
    return config, net.eval()


@pytest.fixture(scope="module")
def tiny():
    return _net("tiny")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return load_golden(golden_dir, "guidance.pt")


class _Spy:
    """Counts the calls of one library entry point made through the ctypes handle."""

    def __init__(self, name):
        from mcvd_pytorch_amd import _lib
        self.lib, self.name, self.real, self.calls = _lib.lib, name, getattr(_lib.lib, name), 0

    def __enter__(self):
        def spy(*a):
            self.calls += 1
            return self.real(*a)
        setattr(self.lib, self.name, spy)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.name, self.real)


def _w(s):
    return float(np.float32(s - 1.0))


def combine_ref(e_c, e_u, s):
    """torch, op by op in fp32: three roundings."""
    d = e_c - e_u
    p = _w(s) * d
    return e_c + p


def update_ref(kind, x, e, z, coef, clip):
    """models/__init__.py:287-290 / :165-168 / :324-328, op by op in fp32 (what sampler_update_kernel restates)."""
    c_x0a, c_x0b, c0, c1, cn = coef
    t = c_x0b * e
    t = x - t
    x0 = c_x0a * t
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    a = c0 * x0
    b = c1 * (x if kind == DDPM else e)
    v = a + b
    if cn != 0.0:
        q = cn * z
        v = v + q
    return v


def _coef(kind):
    f = lambda v: float(np.float32(v))      # noqa: E731
    a, ap = np.float32(0.37), np.float32(0.52)
    b = np.float32(1) - a / ap
    cn = f(np.sqrt((1 - ap) / (1 - a) * b))
    if kind == DDPM:
        return (f(1 / np.sqrt(a)), f(np.sqrt(1 - a)), f(np.sqrt(ap) * b / (1 - a)), f(np.sqrt(1 - b) * (1 - ap) / (1 - a)), cn)
    return (f(1 / np.sqrt(a)), f(np.sqrt(1 - a)), f(np.sqrt(ap)), f(np.sqrt(1 - ap)), cn)


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("B,per", [(1, 64), (2, 64), (3, 64), (1, 2048), (2, 2048), (3, 2048), (1, BIG)])
def test_combine_and_guided_update_kernels_bit_exact(tiny, B, per):
    from mcvd_pytorch_amd import _lib
    net = tiny[1]
    ctx, n, big = net._ctx, B * per, per == BIG
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + per % 997)
    x0 = torch.randn(B, per, device="cuda", generator=g)
    eps2 = torch.randn(2, B, per, device="cuda", generator=g)
    e_c, e_u = eps2[0], eps2[1]
    z_inj = torch.randn(B, per, device="cuda", generator=g)
    seed, off, draw = 77, 5, 3
    z_phi = torch.empty(B, per, device="cuda")
    with torch.cuda.device(net.device):
        net._bind_stream()
        _lib.check(_lib.lib.mcvd_randn(ctx, _ptr(z_phi), C.c_uint64(seed), C.c_uint64(off), C.c_uint64(draw), B, per), "randn")
        for s in SCALES:
            out = torch.empty_like(e_c)
            _lib.check(_lib.lib.mcvd_guidance_combine(ctx, _ptr(out), _ptr(e_c), _ptr(e_u), _w(s), n), "combine")
            assert torch.equal(out, combine_ref(e_c, e_u, s)), f"combine s={s}"
            if s == 1.0:
                assert torch.equal(out, e_c)
        modes = [(DDPM, 1, 2.5, True, True), (DDPM, 1, 2.5, False, False), (DDIM, 0, -0.5, True, False)] if big else \
            itertools.product((DDPM, DDIM), (1, 0), SCALES, (True, False), (True, False))
        for kind, clip, s, philox, dup in modes:
            coef = _coef(kind)
            x = x0.clone()
            xd = torch.full((2, B, per), float("nan"), device="cuda") if dup else None
            _lib.check(_lib.lib.mcvd_sampler_update_guided(
                ctx, kind, _ptr(x), _ptr(xd), _ptr(eps2), None if philox else _ptr(z_inj), _w(s), *coef, clip, n, 1 if philox else 0,
                C.c_uint64(seed), C.c_uint64(off), C.c_uint64(draw), per), "sampler_update_guided")
            want = update_ref(kind, x0, combine_ref(e_c, e_u, s), z_phi if philox else z_inj, coef, clip)
            tag = f"kind={kind} clip={clip} s={s} philox={philox} dup={dup}"
            assert torch.equal(x, want), tag
            if dup:
                assert torch.equal(xd[0], want) and torch.equal(xd[1], want), tag
        # the noise-free form (the last DDPM step, every DDIM step) reads no z at all
        x = x0.clone()
        coef = _coef(DDIM)[:4] + (0.0,)
        _lib.check(_lib.lib.mcvd_sampler_update_guided(ctx, DDIM, _ptr(x), None, _ptr(eps2), None, _w(2.5), *coef, 1, n, 0, C.c_uint64(0),
                                                       C.c_uint64(0), C.c_uint64(0), per), "sampler_update_guided")
        assert torch.equal(x, update_ref(DDIM, x0, combine_ref(e_c, e_u, 2.5), None, coef, 1))


# ------------------------------------------------------------------------------------------------ 2. one guided evaluation
@pytest.mark.parametrize("name,drop", [("tiny", "all"), ("tiny_spade", "past"), ("tiny_spade", "future"), ("tiny_condemb", "all")])
def test_guided_evaluation_is_the_two_halves_of_a_forward_at_2B(name, drop):
    from mcvd_pytorch_amd.runner import guidance_conditioning
    config, net = _net(name)
    B = 2
    x, cond = (t.cuda() for t in synth.make_inputs(config, B, seed=0))
    weak, mask = guidance_conditioning(config, cond, drop)
    labels = torch.tensor([37, 411], device="cuda")
    cmask = torch.tensor([1] * B + [mask] * B, dtype=torch.int32, device="cuda") if config.model.cond_emb else None
    plain = net(torch.cat([x, x]), torch.cat([labels, labels]), cond=torch.cat([cond, weak]), cond_mask=cmask)
    for s in (2.5, 1.0, 0.0):
        got = net(x, labels, cond=cond, guidance_scale=s, guidance_cond=weak, guidance_mask=mask)
        assert torch.equal(got, combine_ref(plain[:B], plain[B:], s)), f"{name} s={s}"
    assert (net(x, labels, cond=cond, guidance_scale=2.5, guidance_cond=weak, guidance_mask=mask) - plain[:B]).abs().max().item() > 1e-3
    if drop == "all":                                         # the default weak conditioning is zeros
        assert torch.equal(net(x, labels, cond=cond, guidance_scale=2.5, guidance_mask=mask), combine_ref(plain[:B], plain[B:], 2.5))
    if name == "tiny":                                        # float timesteps: F-PNDM's midpoint labels
        t = torch.tensor([4.5, 250.0], device="cuda")
        plain_f = net(torch.cat([x, x]), torch.cat([t, t]), cond=torch.cat([cond, weak]))
        assert torch.equal(net(x, t, cond=cond, guidance_scale=2.5, guidance_cond=weak), combine_ref(plain_f[:B], plain_f[B:], 2.5))


def _sampler(kind):
    from mcvd_pytorch_amd.samplers import ddim_sampler, ddpm_sampler, fpndm_sampler
    return dict(ddpm=ddpm_sampler, ddim=ddim_sampler, fpndm=fpndm_sampler)[kind]


def _entry(kind):
    return "mcvd_fpndm_run_guided" if kind == "fpndm" else "mcvd_sampler_run_guided"


def _inputs(config, B, subsample=10):
    x, cond = synth.make_inputs(config, B, seed=0)
    return x.cuda(), cond.cuda(), synth.make_noise(config, B, subsample + 1, seed=2).cuda()


# ------------------------------------------------------------------------------------------------ 3. device loop == host loop
@pytest.mark.parametrize("kind", ["ddpm", "ddim", "fpndm"])
def test_guided_device_loop_equals_host_loop(tiny, kind):
    config, net = tiny
    x, cond, noise = _inputs(config, 2)
    kw = dict(cond=cond, denoise=True, subsample_steps=10, clip_before=True, verbose=False, log=False, guidance_scale=2.5)
    if kind != "fpndm":
        kw["noise"] = noise
    with _Spy(_entry(kind)) as spy:
        dev = _sampler(kind)(x, net, final_only=True, **kw)
        assert spy.calls == 1
        host = _sampler(kind)(x, net, final_only=False, steps_on_device=True, **kw)
        assert spy.calls == 1
    assert torch.equal(dev[0], host[-1])
    plain = _sampler(kind)(x, net, final_only=True, **{k: v for k, v in kw.items() if k != "guidance_scale"})
    assert (dev - plain).abs().max().item() > 1e-2            # the scale moved the frames


# ------------------------------------------------------------------------------------------------ 4. s = 1
@pytest.mark.parametrize("kind", ["ddpm", "ddim", "fpndm"])
def test_scale_one_is_the_unguided_loop_at_2B(tiny, kind):
    config, net = tiny
    B = 2
    x, cond, noise = _inputs(config, B)
    kw = dict(final_only=True, denoise=True, subsample_steps=10, clip_before=True, verbose=False, log=False)
    nz = {} if kind == "fpndm" else dict(noise=noise)
    nz2 = {} if kind == "fpndm" else dict(noise=torch.cat([noise, noise], dim=1).contiguous())
    with _Spy(_entry(kind)) as spy:
        got = _sampler(kind)(x, net, cond=cond, guidance_scale=1.0, **nz, **kw)
        assert spy.calls == 1
    both = _sampler(kind)(torch.cat([x, x]), net, cond=torch.cat([cond, torch.zeros_like(cond)]), **nz2, **kw)
    assert torch.equal(got[0], both[0, :B])
    assert (both[0, :B] - both[0, B:]).abs().max().item() > 1e-2


# ------------------------------------------------------------------------------------------------ 5. the reference's guided runs
N_CASES = 13


@pytest.fixture(scope="module")
def nets():
    """One net per config for the fixture cases (its tuning at the guided batch is found once)."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _net(name)
        return cache[name]
    return get


@pytest.mark.parametrize("i", range(N_CASES))
def test_guided_samplers_vs_reference_golden(fx, nets, i):
    """Gate: the standing 1e-4 on final frames; where that is below 8 x the case's stored fp32-vs-fp64 distance of the reference itself
    (guidance multiplies epsilon errors by up to |s| + |s - 1|), 8 x that distance -- the multiple the metric fixtures use."""
    c = fx["cases"][i]
    name = c["config_name"]
    config, net = nets(name)
    x, cond, noise = fx[f"x_init.{name}"].cuda(), fx[f"cond.{name}"].cuda(), fx[f"noise.{name}"].cuda()
    weak, ref = fx[f"cond_weak.{name}.{c['drop']}"].cuda(), fx[f"result.{name}"][c["row"]]
    kw = dict(cond=cond, final_only=True, denoise=True, subsample_steps=fx["subsample"], clip_before=True, verbose=False, log=False,
              guidance_scale=c["scale"], guidance_cond=weak, guidance_mask=c["mask"])
    if c["kind"] != "fpndm":
        kw.update(noise=noise, t_min=c["t_min"])
    with _Spy(_entry(c["kind"])) as spy:
        out = _sampler(c["kind"])(x, net, **kw)
        assert spy.calls == 1
    err, gate = (out.cpu() - ref).abs().max().item(), max(1e-4, 8.0 * c["ref_dev"])
    print(f"guidance_accuracy {c['id']}: err {err:.3e} gate {gate:.3e} err/gate {err / gate:.3f} ref_dev {c['ref_dev']:.3e}")
    assert err <= gate, f"{c['id']}: {err:.3e} > {gate:.3e}"


# ------------------------------------------------------------------------------------------------ 6. seeded shards
def test_seeded_guided_call_equals_its_shards():
    config, net = _net("tiny")
    x, cond = (t.cuda() for t in synth.make_inputs(config, 3, seed=0))
    kw = dict(final_only=True, denoise=True, subsample_steps=10, clip_before=True, verbose=False, log=False, seed=4242, guidance_scale=2.5,
              t_min=0.3)
    from mcvd_pytorch_amd.samplers import ddpm_sampler
    with _Spy("mcvd_sampler_run_guided") as spy:
        full = ddpm_sampler(x, net, cond=cond, **kw)
        # the shards forward 4 and 2 rows: on the kernels the 6-row call was tuned to, a row's value does not depend on the batch
        net.set_tuning(4, net.get_tuning(6))
        net.set_tuning(2, net.get_tuning(6))
        a = ddpm_sampler(x[:2], net, cond=cond[:2], sample_offset=0, **kw)
        b = ddpm_sampler(x[2:], net, cond=cond[2:], sample_offset=2, **kw)
        assert spy.calls == 3
    assert torch.equal(full[0, :2], a[0]) and torch.equal(full[0, 2:], b[0])
    other = ddpm_sampler(x[2:], net, cond=cond[2:], sample_offset=1, **kw)
    assert not torch.equal(other[0], b[0])                    # the offset keys the stream


# ------------------------------------------------------------------------------------------------ 7. graph replay, old path untouched
def test_second_guided_call_replays_the_graph_and_leaves_the_unguided_path_alone():
    from mcvd_pytorch_amd import _lib
    from mcvd_pytorch_amd.samplers import ddpm_sampler
    config, net = _net("tiny")
    B = 2
    x, cond, noise = _inputs(config, B)
    kw = dict(cond=cond, final_only=True, denoise=True, subsample_steps=10, clip_before=True, verbose=False, log=False, noise=noise)

    def stats():
        cap, rep = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib.mcvd_model_graph_stats(net._model, C.byref(cap), C.byref(rep)))
        return cap.value, rep.value

    def guided():                                             # the library call itself: nothing re-uploads weights in between
        xx = x.clone()
        with torch.cuda.device(net.device):
            net._bind_stream()
            _lib.check(_lib.lib.mcvd_sampler_run_guided(net._model, DDPM, _ptr(xx), _ptr(cond), None, 2.5, 0, _ptr(noise), C.c_uint64(0),
                                                        C.c_uint64(0), 10, _lib.FLAG_DENOISE | _lib.FLAG_CLIP_BEFORE, -1.0, B),
                       "sampler_run_guided")
        return xx

    eager = ddpm_sampler(x, net, guidance_scale=2.5, **kw)[0]
    net.set_option("graph", 1)
    try:
        before = ddpm_sampler(x, net, **kw)[0].clone()
        g1 = guided()
        cap1, rep1 = stats()
        g2 = guided()
        cap2, rep2 = stats()
        after = ddpm_sampler(x, net, **kw)[0]
    finally:
        net.set_option("graph", 0)
    assert cap2 == cap1 and rep2 >= rep1 + 11, ((cap1, rep1), (cap2, rep2))      # 10 steps + the denoise pass, all replayed
    assert torch.equal(g1, g2) and torch.equal(g1, eager)
    assert torch.equal(before, after)


# ------------------------------------------------------------------------------------------------ 8. video_gen
def test_video_gen_rebuilds_the_weak_conditioning_per_block(tiny):
    from mcvd_pytorch_amd.runner import guidance_conditioning, video_gen
    from mcvd_pytorch_amd.samplers import ddpm_sampler
    config, net = tiny
    d = config.data
    Cc, nf, nc = d.channels, d.num_frames, d.num_frames_cond
    x, cond, noise = _inputs(config, 2)
    inits = [torch.randn(x.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(50 + i)) for i in range(2)]
    init_fn = lambda i, shp, dv: inits[i]      # noqa: E731
    with _Spy("mcvd_sampler_run_guided") as spy:
        got = video_gen(config, net, cond, num_frames_pred=2 * nf, task="pred", init_noise_fn=init_fn, sampler=ddpm_sampler, noise=noise,
                        guidance_scale=2.5, guidance_drop="past")
        assert spy.calls == 2
    c, preds = cond, []
    for i in range(2):
        weak, mask = guidance_conditioning(config, c, "past")
        gen = ddpm_sampler(inits[i], net, cond=c, final_only=True, denoise=True, subsample_steps=config.sampling.subsample, clip_before=True,
                           t_min=config.sampling.init_prev_t, verbose=False, log=False, noise=noise, guidance_scale=2.5, guidance_cond=weak,
                           guidance_mask=mask)[-1]
        preds.append(gen)
        c = torch.cat([c[:, Cc * nf:], gen[:, Cc * max(0, nf - nc):]], dim=1).contiguous()
    assert torch.equal(got, torch.cat(preds, dim=1))
    plain = video_gen(config, net, cond, num_frames_pred=2 * nf, task="pred", init_noise_fn=init_fn, sampler=ddpm_sampler, noise=noise)
    assert (got - plain).abs().max().item() > 1e-2


# ------------------------------------------------------------------------------------------------ 9. refusals
@pytest.mark.parametrize("case,kind", [(c, k) for c in ("no_cond_frames", "noise_in_cond", "gamma", "guidance_cond_shape")
                                       for k in ("ddpm", "ddim", "fpndm", "forward") if (c, k) != ("gamma", "forward")])   # gamma is a sampler argument
def test_refusals_come_before_any_launch(case, kind, monkeypatch):
    from mcvd_pytorch_amd import _lib
    name = dict(no_cond_frames="tiny_uncond", noise_in_cond="tiny_noisecond").get(case, "tiny")
    config, net = _net(name)
    x, cond = synth.make_inputs(config, 2, seed=0)
    x, cond = x.cuda(), (cond.cuda() if config.data.num_frames_cond > 0 else None)
    kw = dict(guidance_scale=2.5)
    exc = dict(no_cond_frames=ValueError, noise_in_cond=NotImplementedError, gamma=NotImplementedError, guidance_cond_shape=RuntimeError)[case]
    if case == "gamma":
        kw["gamma"] = True
    if case == "guidance_cond_shape":
        kw["guidance_cond"] = cond[:, :1]

    def launched(*a, **k):
        raise AssertionError("the call reached the device")
    monkeypatch.setattr(net, "sync_parameters", launched)
    for entry in ("mcvd_sampler_run_guided", "mcvd_fpndm_run_guided", "mcvd_unet_forward_guided", "mcvd_unet_forward_guided_ft",
                  "mcvd_sampler_run", "mcvd_fpndm_run", "mcvd_unet_forward"):
        monkeypatch.setattr(_lib.lib, entry, launched)
    with pytest.raises(exc, match="guidance"):
        if kind == "forward":
            net(x, torch.zeros(2, dtype=torch.int64, device="cuda"), cond=cond, **kw)
        else:
            _sampler(kind)(x, net, cond=cond, final_only=True, subsample_steps=10, verbose=False, log=False, **kw)


def test_library_refuses_gamma_and_unconditional_nets(tiny):
    from mcvd_pytorch_amd import _lib
    config, net = tiny
    x, cond, noise = _inputs(config, 2)
    net.sync_parameters(force=True)
    rc = _lib.lib.mcvd_sampler_run_guided(net._model, DDPM, _ptr(x.clone()), _ptr(cond), None, 2.5, 0, _ptr(noise), C.c_uint64(0), C.c_uint64(0),
                                          10, _lib.FLAG_DENOISE | _lib.FLAG_GAMMA, -1.0, 2)
    assert rc == -1 and "GAMMA" in _lib.last_error()
    _, unet = _net("tiny_uncond")
    unet.sync_parameters(force=True)
    xu = synth.make_inputs(synth.make_config("tiny_uncond"), 2, seed=0)[0].cuda()
    rc = _lib.lib.mcvd_sampler_run_guided(unet._model, DDPM, _ptr(xu), None, None, 2.5, 0, _ptr(noise), C.c_uint64(0), C.c_uint64(0), 10,
                                          _lib.FLAG_DENOISE, -1.0, 2)
    assert rc == -1 and "conditioning frames" in _lib.last_error()
