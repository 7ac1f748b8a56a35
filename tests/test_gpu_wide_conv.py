"""GPU: 3x3 convs with 1040 .. 2048 input channels on the K-split Winograd kernels (conv_wino3.cpp ids 11 / 18 / 19, conv_wino2h.cpp 13 / 26,
its one-piece form 25 / 27, conv_wino.cpp 8), whose GroupNorm coefficient table covers the channels of the workgroup's own K part.

Every forced case goes through the stand-alone conv and must RUN the id it names (before the per-part table these launches fell through
every fallback list to a direct tile kernel), with the prologues raw / affine / affine + SiLU over a per-(sample, channel) random table: a
wrong table entry is an O(1) error.  Gates, against an fp64 convolution:
  * ids 8 / 11 / 18 / 19 / 13 / 26: the standing contract 1e-4 * scale + 2e-5 * max(scale, 1);
  * ids 25 / 27: the per-element bound tests/f16x1_ref.py derives for the one-piece arithmetic (+ 2^-23 |bias|); it scales with K;
  * "fp32-accurate", measured and not fixed in advance: on the same data the direct tile kernel (conv_shape 2, unchanged code, what these
    shapes ran before) gives err(tile); the id must stay within  err(id) / mag <= max(2 r err(tile) / mag, floor),  mag = conv(|x|, |w|)
    (ids 13 / 26: the output scale), floor 2e-7 (13 / 26: 1e-6), and r = the worst err(id) / err(tile) over the narrow shapes both kernels
    serve -- (Cin, Cout, H) = (672, 288, 16) and (384, 384, 8), B = 2, the three prologues, this file's data -- R_NARROW below.  The factor 2
    covers the fluctuation of a maximum over elements between shapes.

R_NARROW was measured with measure_ratios() below on an MI355X (tools/wide_conv_accuracy.py); for Cin <= 1024 the launches and their
arithmetic are the parent commit's (the same kernel, the same chunk order, the same reduce pass), so the figures are those of the parent
commit.  Ids 18 / 19 / 26 serve (384, 384, 8) only: 42 chunks do not divide by 4.  The same run, on this file's wide cases
(profiles/wide_conv_accuracy.txt has every line):

    id   r (narrow)   worst wide ratio err(id) / err(tile)   2 r
     8     0.792        0.676  (1152 @16)                    1.583
    11     0.821        0.807  (768 + 576 @16, affine)       1.642
    18     0.430        0.477  (768 + 768 @8)                0.861
    19     0.346        0.296  (2048 @8)                     0.691
    13     0.557        0.560  (768 + 576 @8)                1.115
    26     0.380        0.305  (1152 @16)                    0.760

Every kernel is MORE accurate than the direct tile it replaces (the K split adds partial sums of 1/2 ... 1/8 of the channels); err / mag
stays below 7e-8 everywhere, the floor of 2e-7 never decides.  Ids 25 / 27: worst |err| / max|y| 5.7e-4, inside the derived bound.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from oracle import synth, unet_ref
from tests import f16x1_ref as R

pytestmark = pytest.mark.gpu

WINO_IDS = (4, 8, 10, 11, 12, 13, 16, 17, 18, 19, 20, 24, 25, 26, 27)        # conv_kernels.h: family >= CF_WINO
TWO_PIECE = (12, 13, 26)
TILE = 2                                                                      # conv_shape of the direct tile kernel (64 pixels)

# worst err(id) / err(tile) on the narrow shapes (tools/wide_conv_accuracy.py prints them; profiles/wide_conv_accuracy.txt)
R_NARROW = {8: 0.792, 11: 0.821, 13: 0.557, 18: 0.430, 19: 0.346, 26: 0.380}
NARROW = [(672, 288, 16), (384, 384, 8)]

CASES = [
    # (id, B, C0, C1, Cout, H)
    (11, 3, 1056, 0, 32, 8),        # G8, odd batch (the second sample of the last workgroup clamped), 33 chunks per part
    (11, 2, 768, 576, 96, 16),      # the 1344 seam inside part 1, regions with halos
    (18, 2, 768, 768, 96, 8),       # 1536, four parts, the seam on a part boundary
    (19, 2, 2048, 0, 64, 8),        # the cap, eight parts
    (11, 1, 1050, 0, 32, 16),       # a padded last chunk in the last part, CinP 1056
    (8, 2, 1152, 0, 64, 16),        # fp32 MFMA, one table entry per thread
    (13, 2, 768, 576, 96, 8),       # f16x2
    (26, 2, 1152, 0, 96, 16),
    (25, 3, 1536, 0, 32, 8),        # f16x1
    (27, 2, 1344, 0, 96, 16),
]


@pytest.fixture(scope="module")
def ctx():
    from tests.hiputil import Ctx
    return Ctx()


def _case(B, C0, C1, Cout, H, seed=31):
    """The data of tests/test_gpu_f16x1.py: Gaussian input, weights of unit output variance, a per-(sample, channel) random (A, B) table."""
    g = torch.Generator().manual_seed(seed)
    Cin = C0 + C1
    x = torch.randn(B, Cin, H, H, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    bias = 0.1 * torch.randn(Cout, generator=g)
    coef = torch.stack([(1 + 0.3 * torch.randn(B, Cin, generator=g)), 0.3 * torch.randn(B, Cin, generator=g)], -1).contiguous()
    return x, w, bias, coef


def _run(ctx, shape, x0, x1, w, bias, kw):
    from mcvd_pytorch_amd import _lib
    ctx.opt("conv_shape", shape)
    try:
        y = ctx.conv2d(x0, w, bias, x1=x1, **kw)
        return y, _lib.lib.mcvd_last_conv_kernel()
    finally:
        ctx.opt("conv_shape", -1)


def _errors(ctx, shape, B, C0, C1, Cout, H):
    """Per prologue: (output of `shape`, the id that ran, err(id), err(tile), mag, scale, activated input, y64, data)."""
    x, w, bias, coef = _case(B, C0, C1, Cout, H)
    x0, x1 = (x[:, :C0].contiguous().cuda(), x[:, C0:].contiguous().cuda()) if C1 else (x.cuda(), None)
    wd, bd = w.cuda(), bias.cuda()
    out = []
    for pro in (0, 1, 2):                                        # raw, affine, affine + SiLU
        kw = dict(coef=coef.cuda() if pro else None, act=1 if pro == 2 else 0)
        got, ran = _run(ctx, shape, x0, x1, wd, bd, kw)
        again, _ = _run(ctx, shape, x0, x1, wd, bd, kw)
        tile, ran_tile = _run(ctx, TILE, x0, x1, wd, bd, kw)
        assert 0 <= ran_tile <= 3, ran_tile
        d = R.activate(x, coef if pro else None, pro == 2)
        y64 = F.conv2d(d, w.double(), bias.double(), padding=1)
        mag = F.conv2d(d.abs(), w.double().abs(), None, padding=1).max().item()
        err = (got.cpu().double() - y64).abs()
        err_tile = (tile.cpu().double() - y64).abs().max().item()
        out.append(dict(pro=pro, got=got, again=again, ran=ran, err=err, err_tile=err_tile, mag=mag, scale=y64.abs().max().item(), d=d, y64=y64,
                        w=w, bias=bias))
    return out


def measure_ratios(ctx, shape, cases):
    """[(case, pro, err(id) / err(tile))]: what R_NARROW and profiles/wide_conv_accuracy.txt hold (tools/wide_conv_accuracy.py)."""
    rows = []
    for B, C0, C1, Cout, H in cases:
        for e in _errors(ctx, shape, B, C0, C1, Cout, H):
            rows.append(((B, C0, C1, Cout, H), e["pro"], e["ran"], e["err"].max().item(), e["err_tile"], e["mag"], e["scale"]))
    return rows


@pytest.mark.parametrize("shape,B,C0,C1,Cout,H", CASES, ids=lambda v: str(v))
def test_forced_wide_layer_runs_its_id_and_meets_its_gates(ctx, shape, B, C0, C1, Cout, H):
    for e in _errors(ctx, shape, B, C0, C1, Cout, H):
        pro, got, err = e["pro"], e["got"], e["err"]
        worst, scale, mag = err.max().item(), e["scale"], e["mag"]
        assert e["ran"] == shape, f"forced {shape} at {C0}+{C1} channels, ran {e['ran']}"
        assert torch.isfinite(got).all()
        assert torch.equal(got, e["again"]), f"pro {pro}: two runs differ"
        if shape in (25, 27):
            _, bound = R.wino_f16x1(e["d"], e["w"])
            bound = bound + 2.0 ** -23 * e["bias"].double().abs().reshape(1, -1, 1, 1)
            ratio = (err / bound).max().item()
            print(f"id {shape} B{B} {C0}+{C1}->{Cout} @{H} pro {pro}: worst |err| / bound {ratio:.4f}, max|err| / max|y| {worst / scale:.2e}")
            assert (err <= bound).all(), f"pro {pro}: |err| / bound = {ratio:.3f}"
            assert worst > 1e-5 * scale, "fp32-sized error: one fp16 piece did not run"
            continue
        two_piece = shape in TWO_PIECE
        norm, floor = (scale, 1e-6) if two_piece else (mag, 2e-7)
        print(f"id {shape} B{B} {C0}+{C1}->{Cout} @{H} pro {pro}: err / norm {worst / norm:.3e}, tile {e['err_tile'] / norm:.3e}, "
              f"ratio {worst / e['err_tile']:.3f} (r narrow {R_NARROW[shape]}), max|err| / max|y| {worst / scale:.2e}")
        assert worst <= 1e-4 * scale + 2e-5 * max(scale, 1.0), f"pro {pro}: max-abs err {worst:.3e} (scale {scale:.3e})"
        assert worst / norm <= max(2.0 * R_NARROW[shape] * e["err_tile"] / norm, floor), \
            f"pro {pro}: err {worst / norm:.3e} vs tile {e['err_tile'] / norm:.3e}, r {R_NARROW[shape]}"


@pytest.mark.parametrize("mag", [1e-6, 1e5], ids=["1e-6", "1e5"])
def test_wide_default_kernel_has_the_fp32_range(ctx, mag):
    """test_default_kernels_have_the_fp32_range of tests/test_gpu_parity.py with id 11 at 1536 channels, 8 x 8: raw input, 1e-5 of the scale."""
    g = torch.Generator().manual_seed(41)
    B, Cin, Cout, H = 3, 1536, 96, 8
    x = torch.randn(B, Cin, H, H, generator=g) * mag
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    bias = 0.1 * mag * torch.randn(Cout, generator=g)
    want = F.conv2d(x.double(), w.double(), bias.double(), padding=1)
    got, ran = _run(ctx, 11, x.cuda(), None, w.cuda(), bias.cuda(), {})
    assert ran == 11
    err = ((got.cpu().double() - want).abs().max() / want.abs().max()).item()
    assert err < 1e-5, f"id 11 at magnitude {mag:g}: relative error {err:.3e}"


def test_unsplit_id_falls_back_down_its_list(ctx):
    """conv_shape 10 at 1536 channels: the unsplit kernel refuses (one part of 1536 channels), so does the next of its list (4), and the launch
    ends on a direct tile -- the right result under a lower id, not a wrong one under 10.  Measured: it reports 2 (tile64)."""
    x, w, bias, coef = _case(2, 1536, 0, 64, 8)
    got, ran = _run(ctx, 10, x.cuda(), None, w.cuda(), bias.cuda(), dict(coef=coef.cuda(), act=1))
    print(f"conv_shape 10 at 1536 channels ran {ran}")
    assert ran != 10 and 0 <= ran <= 11, ran
    assert 0 <= ran <= 4, ran                  # (its list is 10, 4; neither takes an unsplit 1536-channel launch: the tile heuristic)
    y64 = F.conv2d(R.activate(x, coef, True), w.double(), bias.double(), padding=1)
    scale = y64.abs().max().item()
    assert (got.cpu().double() - y64).abs().max().item() <= 1e-4 * scale + 2e-5 * max(scale, 1.0)


# ------------------------------------------------------------------------------------------------ a model
def _config(spade):
    """The up path of configs/ucf101.yml at two levels: widths 576 / 768, so 1536 -> 768 and 1344 -> 768 at 8 x 8 and 1344 -> 576 at 16 x 16
    (and the 1x1 shortcuts Conv_2 of the same blocks).  The last block of the 16 x 16 level concatenates the stem's 192 channels, not a
    576-wide skip: 768 -> 576; the 1152 -> 576 layer of the full four-level net is covered by the forced cases above."""
    config = synth.make_config("tiny_spade" if spade else "tiny")
    config.data.image_size = 16
    config.model.ngf = 192
    config.model.n_head_channels = 96
    config.model.ch_mult = [3, 4]
    config.model.num_res_blocks = 1
    config.model.attn_resolutions = [8]
    if spade:
        config.model.spade = True
        config.model.spade_dim = 64
    config.device = "cuda:0"
    return config


def _conv_ops(net):
    """[(op index, ks, H, Cin, Cout, kernel that ran, has a norm in front, module)] of every conv op of the plan."""
    from mcvd_pytorch_amd import _lib
    n = _lib.lib.mcvd_model_profile_read(net._model, None, None, None, None, None, 0)
    info, out = (C.c_int * 8)(), []
    for i in range(n):
        _lib.check(_lib.lib.mcvd_model_op_info(net._model, i, info), "op_info")
        if info[0] == 3:
            out.append((i, info[2], info[3], info[4], info[5], _lib.lib.mcvd_model_op_kernel(net._model, i), bool(info[7]), info[1]))
    return out


def _wide3(ops):
    return [o for o in ops if o[1] == 3 and o[3] > 1024]


def _model(spade):
    from mcvd_pytorch_amd.scorenet import HipScoreNet
    config = _config(spade)
    sd = synth.make_state_dict(config, seed=123)
    net = HipScoreNet(config)
    net.load_state_dict(sd, strict=True)
    x, cond = synth.make_inputs(config, 2, seed=0)
    t = torch.tensor([990, 130])
    with torch.no_grad():
        ref = unet_ref.unet_forward(sd, config, x, t, cond)
    return net.eval(), x.cuda(), t.cuda(), cond.cuda(), ref


def test_wide_model_runs_its_deep_convs_on_winograd_kernels():
    net, x, t, cond, ref = _model(False)
    eps = net(x, t, cond=cond).clone()                      # the autotuned forward
    scale = ref.abs().max().item()
    assert (eps.cpu() - ref).abs().max().item() <= 1e-4 * scale
    ops = _conv_ops(net)
    wide = _wide3(ops)
    print("3x3 convs above 1024 channels (H, Cin, Cout, kernel):", [(o[2], o[3], o[4], o[5]) for o in wide])
    print("1x1 convs above 1024 channels (H, Cin, Cout, kernel):", [(o[2], o[3], o[4], o[5]) for o in ops if o[1] == 1 and o[3] > 1024])
    assert sorted((o[2], o[3], o[4]) for o in wide) == [(8, 1344, 768), (8, 1536, 768), (16, 1344, 576)], wide
    assert all(o[5] in WINO_IDS for o in wide), wide
    net.set_option("graph", 1)                              # eager, captured, replayed: the launches survive capture and replay
    try:
        for _ in range(3):
            assert torch.equal(net(x, t, cond=cond), eps)
    finally:
        net.set_option("graph", 0)
    net.set_option("f16x2", 1)
    try:
        a = net(x, t, cond=cond).clone()
        wide2 = _wide3(_conv_ops(net))
    finally:
        net.set_option("f16x2", 0)
    print("under f16x2:", [(o[2], o[3], o[4], o[5]) for o in wide2])
    assert wide2 and all(o[6] for o in wide2), wide2        # (each of them sits behind a GroupNorm)
    assert all(o[5] in TWO_PIECE for o in wide2), wide2
    assert (a - eps).abs().max().item() <= 2e-5 * eps.abs().max().item()          # the gate of test_f16x2_option_... in tests/test_gpu_parity.py
    assert (a.cpu() - ref).abs().max().item() <= 1e-4 * scale


def test_wide_spade_model_runs_its_deep_convs_on_winograd_kernels():
    """The same widths behind SPADE norms: the convs read the tensor spade_apply materialises (no prologue, no table) and were refused by the
    same `Cin <= 1024`."""
    net, x, t, cond, ref = _model(True)
    eps = net(x, t, cond=cond).clone()
    assert (eps.cpu() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()
    wide = [o for o in _wide3(_conv_ops(net)) if o[7] >= 0]
    print("SPADE net, 3x3 convs above 1024 channels (H, Cin, Cout, kernel):", [(o[2], o[3], o[4], o[5]) for o in wide])
    assert len(wide) == 3 and all(o[5] in WINO_IDS for o in wide), wide
