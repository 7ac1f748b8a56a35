"""GPU: the ngf-288 UCF-101 widths -- 3x3 convs of 2049 .. 2304 input channels on the K-split Winograd ids of four or more parts (18 / 19 / 26 /
27; common.h: WINO_MAX_CIN_K4), their 1x1 shortcuts on the split-operand GEMM, and one-level nets of these widths against the REAL reference
(tests/golden/w288_forward.pt, tools/gen_w288_golden.py; the nets are tests/w288_cases.py's).

The forced stand-alone convs use the data, the prologues (raw / affine / affine + SiLU) and the gates of tests/test_gpu_wide_conv.py, imported:
  * ids 18 / 19 / 26: the standing contract 1e-4 * scale + 2e-5 * max(scale, 1) against an fp64 convolution, and
    err(id) / mag <= max(2 r err(tile) / mag, floor) with that file's R_NARROW (18: 0.430, 19: 0.346, 26: 0.380) and floors;
  * id 27: the per-element bound tests/f16x1_ref.py derives.
The ratios err(id) / err(tile) are measured, not fixed in advance: every one is printed (tools/w288_accuracy.py writes them to
profiles/w288_accuracy.txt).

Measured on an MI355X (profiles/w288_accuracy.txt has every line), worst err(id) / err(tile) over the three prologues:
    18 @ 1152 + 1152, 8 x 8: 0.430    18 @ 2290, 16 x 16: 0.382    19 @ 2304: 0.275    19 @ 1152 + 1024: 0.315    26 @ 2304: 0.313   (2 r: 0.86 / 0.69 / 0.76)
    27 @ 1152 + 1152: |err| at most 0.005 of its derived bound, 5.7e-4 of max |y|.

The model cases fail on the parent commit, where HipScoreNet(config) raises "desc: ngf=288".
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from oracle import sampler_ref, synth, unet_ref
from tests import f16x1_ref as R
from tests import test_gpu_wide_conv as T
from tests import w288_cases as W

pytestmark = pytest.mark.gpu

CASES = [
    # (id, B, C0, C1, Cout, H)
    (18, 2, 1152, 1152, 96, 8),     # 2304, four parts of 36 chunks, the seam on a part boundary
    (19, 3, 2304, 0, 32, 8),        # eight parts of 18 chunks, odd batch under G8
    (19, 2, 1152, 1024, 64, 8),     # 2176 = 136 chunks, the seam inside a part
    (18, 1, 2290, 0, 32, 16),       # CinP 2304 with a padded last chunk, regions with halos
    (26, 2, 2304, 0, 96, 8),        # f16x2 four-way
    (27, 2, 1152, 1152, 96, 8),     # f16x1 four-way
]
OP_ATTN = 5                         # model.h: OpKind (tests/test_gpu_attention_wide.py)
AK_WIDE2, AK_WIDE3 = 5, 6           # attn_kernels.h


@pytest.fixture(scope="module")
def ctx():
    from tests.hiputil import Ctx
    return Ctx()


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return W.load(golden_dir)


# ------------------------------------------------------------------------------------------------ forced stand-alone convs
@pytest.mark.parametrize("shape,B,C0,C1,Cout,H", CASES, ids=lambda v: str(v))
def test_forced_layer_above_2048_channels_runs_its_id_and_meets_its_gates(ctx, shape, B, C0, C1, Cout, H):
    for e in T._errors(ctx, shape, B, C0, C1, Cout, H):
        pro, got, err = e["pro"], e["got"], e["err"]
        worst, scale, mag = err.max().item(), e["scale"], e["mag"]
        assert e["ran"] == shape, f"forced {shape} at {C0}+{C1} channels, ran {e['ran']}"
        assert torch.isfinite(got).all()
        assert torch.equal(got, e["again"]), f"pro {pro}: two runs differ"
        if shape == 27:
            _, bound = R.wino_f16x1(e["d"], e["w"])
            bound = bound + 2.0 ** -23 * e["bias"].double().abs().reshape(1, -1, 1, 1)
            ratio = (err / bound).max().item()
            print(f"id {shape} B{B} {C0}+{C1}->{Cout} @{H} pro {pro}: worst |err| / bound {ratio:.4f}, max|err| / max|y| {worst / scale:.2e}, "
                  f"ratio to the tile {worst / e['err_tile']:.1f}")
            assert (err <= bound).all(), f"pro {pro}: |err| / bound = {ratio:.3f}"
            assert worst > 1e-5 * scale, "fp32-sized error: one fp16 piece did not run"
            continue
        norm, floor = (scale, 1e-6) if shape in T.TWO_PIECE else (mag, 2e-7)
        print(f"id {shape} B{B} {C0}+{C1}->{Cout} @{H} pro {pro}: err / norm {worst / norm:.3e}, tile {e['err_tile'] / norm:.3e}, "
              f"ratio {worst / e['err_tile']:.3f} (r narrow {T.R_NARROW[shape]}), max|err| / max|y| {worst / scale:.2e}")
        assert worst <= 1e-4 * scale + 2e-5 * max(scale, 1.0), f"pro {pro}: max-abs err {worst:.3e} (scale {scale:.3e})"
        assert worst / norm <= max(2.0 * T.R_NARROW[shape] * e["err_tile"] / norm, floor), \
            f"pro {pro}: err {worst / norm:.3e} vs tile {e['err_tile'] / norm:.3e}, r {T.R_NARROW[shape]}"


@pytest.mark.parametrize("shape,Cin", [(11, 2304), (19, 2320)], ids=["11@2304", "19@2320"])
def test_refused_launches_end_on_a_kernel_outside_the_winograd_ids(ctx, shape, Cin):
    """The 2-way split at 2304 channels (1152 per part: more than the table) and anything above 2304: every id of the fallback list refuses,
    and the launch ends on a direct tile with the right result."""
    x, w, bias, coef = T._case(2, Cin, 0, 32, 8)
    got, ran = T._run(ctx, shape, x.cuda(), None, w.cuda(), bias.cuda(), dict(coef=coef.cuda(), act=1))
    print(f"conv_shape {shape} at {Cin} channels ran {ran}")
    assert ran not in T.WINO_IDS and 0 <= ran <= 3, ran
    y64 = F.conv2d(R.activate(x, coef, True), w.double(), bias.double(), padding=1)
    scale = y64.abs().max().item()
    assert (got.cpu().double() - y64).abs().max().item() <= 1e-4 * scale + 2e-5 * max(scale, 1.0)


@pytest.mark.parametrize("H", [8, 16])
@pytest.mark.parametrize("shape", [15, 14])
def test_forced_1x1_over_the_2304_channel_concat(ctx, shape, H):
    """The shortcut Conv_2 of the 2304-channel blocks as a stand-alone launch: 1152 + 1152 -> 96, B = 2, affine prologue, ids 15 (three bf16
    pieces) / 14 (two fp16 pieces) at every cout tile that divides 96 / 32.  The per-image coefficient table fills the LDS at this width
    (conv1x1_h2.cpp: q1_lds_bytes against 80 KB): at least tile 1 must take the launch; the tiles that did are printed.  Then the same launch
    over the RAW concat, which is what the shortcut reads in a model: no prologue, no table, and cout tile 3 fits as well."""
    g = torch.Generator().manual_seed(53)
    B, C0, C1, Cout = 2, 1152, 1152, 96
    x = torch.randn(B, C0 + C1, H, H, generator=g)
    w = torch.randn(Cout, C0 + C1, 1, 1, generator=g) / (C0 + C1) ** 0.5
    bias = 0.1 * torch.randn(Cout, generator=g)
    coef = torch.stack([(1 + 0.3 * torch.randn(B, C0 + C1, generator=g)), 0.3 * torch.randn(B, C0 + C1, generator=g)], -1).contiguous()
    x0, x1 = x[:, :C0].contiguous().cuda(), x[:, C0:].contiguous().cuda()
    for pro in ("affine", "raw"):
        y64 = F.conv2d(R.activate(x, coef if pro == "affine" else None, False), w.double(), bias.double())
        scale = y64.abs().max().item()
        usable = []
        for cot in (1, 3):
            ctx.opt("conv_cot", cot)
            try:
                got, ran = T._run(ctx, shape, x0, x1, w.cuda(), bias.cuda(), dict(coef=coef.cuda() if pro == "affine" else None, act=0))
            finally:
                ctx.opt("conv_cot", 0)
            err = (got.cpu().double() - y64).abs().max().item()
            print(f"id {shape} 1152+1152->96 @{H} {pro} cout tile {cot}: ran {ran}, max-abs err {err:.3e} (scale {scale:.3f})")
            assert err <= 1e-4 * scale + 2e-5 * max(scale, 1.0), (pro, cot, ran, err)
            assert ran == shape or 0 <= ran <= 3, ran           # the id, or refused (LDS) and a direct tile
            if ran == shape:
                usable.append(cot)
        print(f"id {shape} @{H} {pro}: usable cout tiles {usable}")
        assert 1 in usable, (pro, usable)
        if pro == "raw":
            assert usable == [1, 3], usable                     # 4 * 3 * np * 256 + 4 * 16 * 128 floats: 69 KB (np = 3) of the 80 KB budget


# ------------------------------------------------------------------------------------------------ the model
def _attn_ops(net):
    from mcvd_pytorch_amd import _lib
    n = _lib.lib.mcvd_model_profile_read(net._model, None, None, None, None, None, 0)
    info, out = (C.c_int * 8)(), []
    for i in range(n):
        _lib.check(_lib.lib.mcvd_model_op_info(net._model, i, info), "op_info")
        if info[0] == OP_ATTN:
            out.append(_lib.lib.mcvd_model_op_attention_kernel(net._model, i))
    return out


_NETS = {}


def _net(case):
    """One HipScoreNet per case and module run (the weights are 0.4 GB of synthetic draws: built once)."""
    if case not in _NETS:
        from mcvd_pytorch_amd.scorenet import HipScoreNet
        config = W.make_config(case)
        config.device = "cuda:0"
        sd = synth.make_state_dict(config, seed=W.SEED)
        net = HipScoreNet(config)             # the parent commit raises here: "desc: ngf=288"
        net.load_state_dict(sd, strict=True)
        _NETS[case] = (config, sd, net.eval())
    return _NETS[case]


def _wide3(ops):
    """The 3x3 convs of a module over the two concats, 1152 + 1152 and 1152 + 288 (tests/test_gpu_wide_conv.py: _conv_ops tuples)."""
    return [o for o in ops if o[1] == 3 and o[3] in (1440, 2304) and o[7] >= 0]


def _forward(net, g):
    mask = g.get("mask")
    return net(g["x"].cuda(), g["t"].cuda(), cond=g["cond"].cuda(), cond_mask=mask.cuda() if mask is not None else None).clone()


@pytest.mark.parametrize("case", W.CASES)
def test_w288_model_matches_the_reference_on_matrix_pipe_kernels(fixture, case):
    from tests.hiputil import module_output
    g = fixture[case]
    config, sd, net = _net(case)
    eps = _forward(net, g)                                   # the autotuned forward, no option set
    ref = g["eps"]
    scale = ref.abs().max().item()
    err = (eps.cpu() - ref).abs().max().item()
    print(f"{case}: |eps - reference| {err:.3e} of max {scale:.3f}")
    assert err <= 1e-4 * scale
    temb = module_output(net, 1, g["batch"]).cpu()           # module 1 holds SiLU(temb) (include/mcvd_hip.h)
    want = unet_ref.silu(g["tap_temb"])
    assert (temb[:, :1152] - want).abs().max().item() <= 1e-4 * want.abs().max().item()
    up = module_output(net, g["up_block"], g["batch"]).cpu()
    assert list(up.shape) == [g["batch"], 1152, 8, 8]
    assert (up.reshape(-1)[::W.TAP_STRIDE] - g["tap_up"]).abs().max().item() <= 1e-4 * g["tap_up_scale"]
    # what ran
    ops = T._conv_ops(net)
    wide = _wide3(ops)
    wide1 = [o for o in ops if o[1] == 1 and o[3] > 1024]
    attn = _attn_ops(net)
    print(f"{case}: 3x3 convs above 1024 channels (H, Cin, Cout, kernel):", [(o[2], o[3], o[4], o[5]) for o in ops if o[1] == 3 and o[3] > 1024])
    print(f"{case}: 1x1 convs above 1024 channels (H, Cin, Cout, kernel):", [(o[2], o[3], o[4], o[5]) for o in wide1])
    print(f"{case}: attention kernels:", attn)
    assert sorted((o[2], o[3], o[4]) for o in wide) == [(8, 1440, 1152), (8, 2304, 1152)], wide
    assert all(o[5] in T.WINO_IDS for o in wide), wide
    assert all(o[5] in (18, 19) for o in wide if o[3] == 2304), wide
    # (SPADE case: spade_apply materialises the normalised tensor -- the fused loader stops at 1024 channels -- and the convs read it plainly)
    assert sorted((o[3], o[4]) for o in wide1 if o[4] == 1152 and o[3] > 1152) == [(1440, 1152), (2304, 1152)], wide1
    assert len(wide1) >= 2 + 3 * 2, wide1                    # the two shortcuts, q|k|v and NIN_3 of three attention blocks
    assert len(attn) == 3 and all(k == AK_WIDE3 for k in attn), attn
    net.set_option("graph", 1)                               # eager, captured, replayed
    try:
        for _ in range(3):
            assert torch.equal(_forward(net, g), eps)
    finally:
        net.set_option("graph", 0)


@pytest.mark.parametrize("case", W.CASES)
def test_w288_model_runs_its_wide_1x1_gemms_off_the_direct_tile(fixture, case):
    """Every 1x1 op above 1024 input channels -- the two shortcuts Conv_2 (2304 -> 1152, 1440 -> 1152), q|k|v (1152 -> 3456) and NIN_3 (1152 -> 1152) of
    the three attention blocks -- must run a kernel other than a direct tile in the autotuned forward at the fixture's batch, B = 2.

    At B = 2 an 8 x 8 plane is 128 pixels, ONE pixel tile of the split-operand GEMM, and its block map put every working workgroup of such a launch
    on one XCD: q|k|v then lost to the direct tile, which spreads (id 15 at cout tile 64 / 32: 61.7 / 86.6 us against tile64's 46.0, median of 9
    forwards on an MI355X).  With fewer than eight pixel tiles the launch now covers all XCDs (conv1x1_h2.cpp); measured the same way, us (id / cout tile):
        1152 -> 3456 (q|k|v, affine prologue)   15 / 1  34.3   15 / 2  41.1   tile64 / 1  45.9
        1152 -> 1152 (NIN_3, raw)               15 / 1  27.8   15 / 2  35.2   tile64 / 1  53.9
        2304 -> 1152 (Conv_2, raw)              15 / 1  47.8   15 / 2  60.6   tile64 / 1  81.6
        1440 -> 1152 (Conv_2, raw)              15 / 1  32.7   15 / 2  41.3   tile64 / 1  53.5"""
    config, sd, net = _net(case)
    _forward(net, fixture[case])
    wide1 = [o for o in T._conv_ops(net) if o[1] == 1 and o[3] > 1024]
    print(f"{case}: 1x1 convs above 1024 channels (H, Cin, Cout, kernel):", [(o[2], o[3], o[4], o[5]) for o in wide1])
    assert len(wide1) >= 8
    assert all(o[5] > 3 for o in wide1 if o[4] != 3 * o[3]), wide1          # the shortcuts and NIN_3
    assert all(o[5] > 3 for o in wide1), wide1


def test_w288_model_under_f16x2_and_f16x1(fixture):
    from mcvd_pytorch_amd import _lib
    g = fixture["plain"]
    config, sd, net = _net("plain")
    eps = _forward(net, g)
    ref = g["eps"]
    net.set_option("f16x2", 1)
    try:
        a = _forward(net, g)
        wide2 = _wide3(T._conv_ops(net))
    finally:
        net.set_option("f16x2", 0)
    print("under f16x2:", [(o[2], o[3], o[4], o[5]) for o in wide2])
    assert len(wide2) == 2 and all(o[6] for o in wide2), wide2              # (each of them sits behind a GroupNorm)
    assert all(o[5] in T.TWO_PIECE for o in wide2), wide2
    assert all(o[5] == 26 for o in wide2 if o[3] == 2304), wide2
    print(f"f16x2: |eps - default| / max {(a - eps).abs().max().item() / eps.abs().max().item():.3e}")
    assert (a - eps).abs().max().item() <= 2e-5 * eps.abs().max().item()          # the gate of tests/test_gpu_wide_conv.py
    assert (a.cpu() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()
    net.set_option("f16x1", 1)
    try:
        b = _forward(net, g)
        wide1h = _wide3(T._conv_ops(net))
        rng = _lib.lib.mcvd_ctx_check_range(net._ctx)
    finally:
        net.set_option("f16x1", 0)
    print("under f16x1:", [(o[2], o[3], o[4], o[5]) for o in wide1h],
          f"|eps - default| / max {(b - eps).abs().max().item() / eps.abs().max().item():.3e}")
    assert rng == 0 and torch.isfinite(b).all()
    assert len(wide1h) == 2 and all(o[5] in (25, 27) for o in wide1h), wide1h
    assert all(o[5] == 27 for o in wide1h if o[3] == 2304), wide1h
    c = _forward(net, g)                                                     # the options off again: re-tuned, the default arithmetic
    assert (c.cpu() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()
    assert all(o[5] not in (12, 13, 24, 25, 26, 27) for o in T._conv_ops(net)), "an fp16 Winograd id ran with both options off"


def test_w288_ddpm_sampler_matches_the_oracle(fixture):
    """DDPM, subsample_steps = 5, denoise, injected noise: the device loop against oracle/sampler_ref.py (which tests/test_w288_cpu.py holds to
    the reference's own sampler at this width), 1e-4 on frames in [-1, 1]."""
    from mcvd_pytorch_amd.samplers import ddpm_sampler
    g = fixture["plain"]
    config, sd, net = _net("plain")
    noise = synth.make_noise(config, g["batch"], 6, seed=2)
    k = [0]

    def fn(i, like):
        k[0] += 1
        return noise[k[0] - 1]
    torch.set_num_threads(16)
    want = sampler_ref.sample(g["x"].clone(), unet_ref.OracleScoreNet(config, sd), cond=g["cond"], kind="ddpm", final_only=True, denoise=True,
                              subsample_steps=5, clip_before=True, noise_fn=fn)
    got = ddpm_sampler(g["x"].cuda(), net, cond=g["cond"].cuda(), final_only=True, denoise=True, subsample_steps=5, noise=noise.cuda())
    assert got.shape == want.shape
    err = (got.cpu() - want).abs().max().item()
    print(f"DDPM-5 + denoise: |device - oracle| {err:.3e}; |device - reference| {(got.cpu() - g['sampler_ddpm5']).abs().max().item():.3e}")
    assert err <= 1e-4
