"""GPU: the wide-head attention kernel (attention_wide.cpp: head dims 160 ... 1024, the head dim divided over the waves of a workgroup) and
the dispatch table that sends launches to it (attn_kernels.h), through mcvd_op_attention and through a model whose attention blocks have
one head over all channels of the level (model.n_head_channels = -1, layerspp.py:221-228).

Gate: the project's standing attention gate, err <= 1e-4 scale + 2e-5 max(scale, 1) with scale = max|want| (tests/test_gpu_parity.py
_close, restated here), against softmax attention in fp64 (layerspp.py:237-244)."""
import ctypes as C

import pytest
import torch

from oracle import synth, unet_ref

pytestmark = pytest.mark.gpu

AK_NAIVE, AK_FLASH_F32, AK_SPLIT2, AK_SPLIT3, AK_SPLIT3_PRESPLIT, AK_WIDE2, AK_WIDE3 = range(7)
OP_ATTN = 5


def _gate(want, rtol=1e-4, atol=2e-5):
    scale = max(want.abs().max().item(), 1e-6)
    return atol * max(scale, 1.0) + rtol * scale


def _err(got, want):
    got = got.detach().float().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return (got - want.float()).abs().max().item()


@pytest.fixture(scope="module")
def ctx():
    from tests.hiputil import Ctx
    return Ctx()


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _ran():
    from mcvd_pytorch_amd import _lib
    return _lib.lib.mcvd_last_attention_kernel()


def _attn_ref(qkv, heads, dtype=torch.float64):
    B, C3, S = qkv.shape
    Cc = C3 // 3
    D = Cc // heads
    q, k, v = (qkv[:, i * Cc:(i + 1) * Cc].to(dtype).reshape(B * heads, D, S) for i in range(3))
    w = torch.softmax(torch.matmul(q.transpose(1, 2), k) * (int(D) ** (-0.5)), dim=-1)
    return torch.matmul(v, w.transpose(1, 2)).reshape(B, Cc, S)


def _randn_case(B, Cc, S, seed=9):
    qkv = torch.randn(B, 3 * Cc, S, generator=_g(seed))
    qkv[:, :Cc] *= 1.5           # as test_attention: a softmax peaky enough to exercise the online rescale
    return qkv


def _run(ctx, qkv, heads, mode, f16x2=0):
    ctx.opt("f16x2", f16x2)
    ctx.opt("naive_attn", mode)
    try:
        got = ctx.attention(qkv.cuda(), heads)
        torch.cuda.synchronize()
        return got.cpu(), _ran()
    finally:
        ctx.opt("naive_attn", 0)
        ctx.opt("f16x2", 0)


# ------------------------------------------------------------------------------------------------ 1. dispatch
@pytest.mark.parametrize("Cc,H,mode,f16x2,want", [
    (384, 8, 0, 0, AK_WIDE3),          # default options
    (384, 8, 0, 1, AK_WIDE2),          # option f16x2
    (384, 8, 1, 0, AK_NAIVE),
    (384, 8, 2, 0, AK_NAIVE),          # the dispatch before the wide kernel: no fp32 flash kernel beyond 256
    (192, 8, 2, 0, AK_FLASH_F32),
    (48, 8, 0, 0, AK_NAIVE),           # head dim no multiple of 32
    (384, 4, 0, 0, AK_NAIVE),          # 16 tokens: no multiple of 32
    (96, 8, 0, 0, AK_SPLIT3),          # as before
    (192, 16, 0, 0, AK_WIDE3),         # 160 ... 256, the measured verdict (attn_kernels.h): three pieces wide up to 256 tokens ...
    (192, 32, 0, 0, AK_FLASH_F32),     # ... the fp32 flash kernel beyond
    (192, 32, 0, 1, AK_WIDE2),         # ... two pieces wide at every token count
])
def test_dispatch(ctx, Cc, H, mode, f16x2, want):
    qkv = _randn_case(1, Cc, H * H)
    got, ran = _run(ctx, qkv, 1, mode, f16x2)
    assert ran == want, (ran, want)
    assert _err(got, _attn_ref(qkv, 1)) <= _gate(_attn_ref(qkv, 1))


# ------------------------------------------------------------------------------------------------ 2. accuracy against fp64
CASES = [(1, 160, 1, 8),        # five channel tiles: uneven slices, three waves without channels
         (2, 288, 1, 8),        # nine tiles: one wave with two; two key tiles
         (1, 320, 1, 16),
         (2, 384, 1, 8),
         (3, 576, 2, 16),       # head dim 288, two heads; B * heads = 6 is no multiple of the 8 XCD slots
         (1, 768, 1, 8),
         (1, 1024, 1, 16),      # the cap
         (1, 384, 1, 32),       # 32 key tiles, 32 query tiles
         (5, 192, 1, 8),        # 160 ... 256: the table sends them to the wide kernel (attn_kernels.h AK_WIDE_FROM_D)
         (1, 256, 1, 8)]


@pytest.fixture(scope="module")
def refs():
    """(qkv, fp64 attention) per case, computed once and shared by the two modes."""
    out = {}
    for case in CASES:
        B, Cc, heads, H = case
        qkv = _randn_case(B, Cc, H * H)
        out[case] = (qkv, _attn_ref(qkv, heads))
    return out


@pytest.mark.parametrize("mode", [4, 3], ids=["bf16x3", "f16x2"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d_C%d_h%d_%dx%d" % (c[0], c[1], c[2], c[3], c[3]))
def test_accuracy(ctx, refs, case, mode):
    qkv, want = refs[case]
    got, ran = _run(ctx, qkv, case[2], mode)
    assert ran == (AK_WIDE3 if mode == 4 else AK_WIDE2), ran
    err, gate = _err(got, want), _gate(want)
    print(f"wide attention {case} mode {mode}: err {err:.3e} = {err / gate:.3f} of the gate")
    assert err <= gate, f"max-abs err {err:.3e} > {gate:.3e}"


# ------------------------------------------------------------------------------------------------ 3. the softmax walked
def _walk_inputs(pattern, D, carrier):
    """test_attention_lazy_softmax_reference's score profiles, B = 1, one head, 16 x 16; the scores ride on channel `carrier`."""
    g = _g(21)
    S = 256
    v = torch.randn(1, D, S, generator=g)
    tile = torch.arange(S).float() // 32
    if pattern == "ramp_up":
        prof = 21.0 * tile + 0.5 * torch.randn(S, generator=g)          # natural-log units: 30.3 in base 2 per key tile
    elif pattern == "ramp_down":
        prof = -21.0 * tile + 0.5 * torch.randn(S, generator=g)
    elif pattern == "spike_late":
        prof = torch.randn(S, generator=g); prof[S - 3] = 300.0
    elif pattern == "flat":
        prof = torch.full((S,), 7.0)
    else:
        prof = torch.randn(S, generator=g); prof[:32] += 200.0
    q = 0.05 * torch.randn(1, D, S, generator=g)
    k = 0.05 * torch.randn(1, D, S, generator=g)
    q[:, carrier] = D ** 0.5                                              # so that scale * q = 1
    k[:, carrier] = prof
    return torch.cat([q, k, v], dim=1)


@pytest.mark.parametrize("pattern", ["ramp_up", "ramp_down", "spike_late", "flat", "huge_first"])
@pytest.mark.parametrize("D", [320, 768])
def test_softmax_walk(ctx, pattern, D):
    """The lazy exponent reference walked as test_attention_lazy_softmax_reference walks it, with the scores carried once by channel 0 (the
    first wave's slice) and once by channel D - 1 (the last wave's: a partial that arrives late or is added twice shows).  Scores of 200 - 300
    carry half an fp32 ulp of 1e-5 in ANY fp32 evaluation, so the gate is relative: 8 x the deviation of torch's own fp32 CPU attention from
    the fp64 result on the same inputs (the margin the LPIPS, FVD and Inception paths get over the reference's rounding), or the fixed gate
    where that is larger."""
    worst = 0.0
    for carrier in (0, D - 1):
        qkv = _walk_inputs(pattern, D, carrier)
        want = _attn_ref(qkv, 1)
        ref_dev = (_attn_ref(qkv, 1, torch.float32).double() - want).abs().max().item()
        got, ran = _run(ctx, qkv, 1, 4)
        assert ran == AK_WIDE3
        assert torch.isfinite(got).all()
        err = _err(got, want)
        worst = max(worst, err / max(ref_dev, 1e-30))
        print(f"softmax walk {pattern} D {D} carrier {carrier}: err {err:.3e}, ref_dev {ref_dev:.3e}, err / ref_dev {err / max(ref_dev, 1e-30):.2f}, "
              f"fixed gate {_gate(want):.3e}")
        assert err <= max(8.0 * ref_dev, _gate(want)), (pattern, D, carrier, err, ref_dev)
    print(f"softmax walk {pattern} D {D}: worst err / ref_dev {worst:.2f}")


# ------------------------------------------------------------------------------------------------ 4. determinism, batch independence
@pytest.mark.parametrize("mode", [4, 3], ids=["bf16x3", "f16x2"])
def test_bit_identical_runs_and_rows(ctx, mode):
    qkv = _randn_case(3, 384, 64, seed=5)
    a, ran = _run(ctx, qkv, 1, mode)
    assert ran == (AK_WIDE3 if mode == 4 else AK_WIDE2)
    b, _ = _run(ctx, qkv, 1, mode)
    assert torch.equal(a, b)
    for i in range(3):
        row, _ = _run(ctx, qkv[i:i + 1].contiguous(), 1, mode)
        assert torch.equal(row[0], a[i]), i


# ------------------------------------------------------------------------------------------------ 5. a model
def _attn_ops(net):
    from mcvd_pytorch_amd import _lib
    n = _lib.lib.mcvd_model_profile_read(net._model, None, None, None, None, None, 0)
    info, out = (C.c_int * 8)(), []
    for i in range(n):
        _lib.check(_lib.lib.mcvd_model_op_info(net._model, i, info), "op_info")
        k = _lib.lib.mcvd_model_op_attention_kernel(net._model, i)
        if info[0] == OP_ATTN:
            out.append(k)
        else:
            assert k == -1, (i, info[0], k)
    return out


def test_single_wide_head_model():
    """tiny with ngf = 160 and n_head_channels = -1: 320-channel single heads at 16 x 16 and 8 x 8."""
    from mcvd_pytorch_amd.scorenet import HipScoreNet
    config = synth.make_config("tiny")
    config.model.ngf = 160
    config.model.n_head_channels = -1
    config.device = "cuda:0"
    sd = synth.make_state_dict(config, seed=123)
    net = HipScoreNet(config)
    net.load_state_dict(sd, strict=True)
    x, cond = synth.make_inputs(config, 2, seed=0)
    t = torch.tensor([990, 130])
    xc, tc, cc = x.cuda(), t.cuda(), cond.cuda()
    eps = net(xc, tc, cond=cc).clone()
    with torch.no_grad():
        ref = unet_ref.unet_forward(sd, config, x, t, cond)
    scale = ref.abs().max().item()
    assert (eps.cpu() - ref).abs().max().item() <= 1e-4 * scale
    kernels = _attn_ops(net)
    assert kernels and all(k == AK_WIDE3 for k in kernels), kernels
    net.set_option("graph", 1)              # eager, captured, replayed: the kernel and its LDS attribute survive capture and replay
    try:
        for _ in range(3):
            again = net(xc, tc, cond=cc).clone()
            assert torch.equal(again, eps)
    finally:
        net.set_option("graph", 0)
    net.set_option("naive_attn", 1)
    try:
        naive = net(xc, tc, cond=cc).clone()
        assert all(k == AK_NAIVE for k in _attn_ops(net))
    finally:
        net.set_option("naive_attn", 0)
    assert (naive - eps).abs().max().item() <= 2e-5 * scale


# ------------------------------------------------------------------------------------------------ 6. f16x2 range
def test_f16x2_range(ctx):
    """Nothing is clamped: a q of 1e5 (times 2^4: beyond fp16) makes the two-piece kernel's output non-finite -- what the model's range guard
    reports as MCVD_ERANGE; the three-piece kernel has the fp32 range."""
    qkv = _randn_case(1, 384, 64, seed=7)
    qkv[0, 17, 5] = 1e5
    want = _attn_ref(qkv, 1)
    got2, ran2 = _run(ctx, qkv, 1, 3)
    assert ran2 == AK_WIDE2 and not torch.isfinite(got2).all()
    got3, ran3 = _run(ctx, qkv, 1, 4)
    assert ran3 == AK_WIDE3 and torch.isfinite(got3).all()
    assert _err(got3, want) <= _gate(want)
