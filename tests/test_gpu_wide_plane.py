"""GPU: 3x3 convs with 1040 .. 2048 input channels on the UNSPLIT Winograd kernels, on planes of 16 x 16 and larger (conv_wino3.cpp id 10,
conv_wino2h.cpp ids 12 / 24, conv_wino.cpp id 4), whose GroupNorm coefficient table now holds up to WINO_TABLE_CH_PLANE = 2048 channels of the
workgroup's one sample (four entries per thread; conv_wino.cpp: two).  No K-split scratch is involved, so a model's 32 x 32 layers above 1024
channels leave the direct tile kernel as well.

Every forced case goes through the stand-alone conv with the data, the three prologues (raw / affine / affine + SiLU over a per-(sample, channel)
random table: a wrong table entry is an O(1) error) and the gates of tests/test_gpu_wide_conv.py, imported, and must RUN the id it names: on the
commit before, these launches fell through every fallback list to a direct tile.  Gates, against an fp64 convolution:
  * ids 10 / 12 / 4: the standing contract 1e-4 * scale + 2e-5 * max(scale, 1);
  * id 24: the per-element bound tests/f16x1_ref.py derives for the one-piece arithmetic (+ 2^-23 |bias|), and an error above 1e-5 of the scale;
  * "fp32-accurate" for ids 10 / 12 / 4, measured and not fixed in advance:  err(id) / norm <= max(2 r err(tile) / norm, floor)  with the norms
    and floors of tests/test_gpu_wide_conv.py (10 / 4: mag = conv(|x|, |w|), 2e-7; 12: the output scale, 1e-6) and r = the worst
    err(id) / err(tile) over the narrow shapes both kernels serve, at 16 x 16: (Cin, Cout, H) = (672, 288, 16) and (384, 384, 16), B = 2, the
    three prologues, this data.  For Cin <= 1024 these launches are the arithmetic of the commit before (the same kernel and chunk order; the
    extra table entries are behind a branch such a launch never takes), so r is a property of unchanged code.

R_PLANE was measured with tools/wide_plane_accuracy.py on an MI355X (profiles/wide_plane_accuracy.txt has every line), with the same run's
worst ratio on this file's wide cases:

    id   r (narrow, 16 x 16)   worst wide ratio err(id) / err(tile)   2 r
    10     1.166                 1.232  (1040 @16, raw)                 2.331
    12     0.763                 0.665  (1152 @16, affine + SiLU)       1.526
     4     1.130                 1.027  (1152 @16, affine)              2.260

The unsplit kernels contract all channels in one accumulator, as the direct tile does: the ratios sit round 1 (the K splits of
tests/test_gpu_wide_conv.py, which add partial sums, are at 0.3 .. 0.8); err / mag stays below 1.1e-7 everywhere.  Id 24: |err| at most 0.009 of
its derived bound, 5.3e-4 of max |y|.

The 2-way split at 2304 channels (1152 per part) would fit a plane's table, but `Cin <= WINO_MAX_CIN` for splits of fewer than four parts stays
in the rule (common.h; tests/test_w288_cpu.py pins the expression), so that launch is not affected: it is among the refusals below, not the cases.
tests/hiputil.py does not expose the SPADE prologue inputs (ConvArgs::gb), so the refusal of id 4 with them set at 1152 channels is not here;
tests/test_wide_plane_cpu.py asserts the predicate.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import synth, unet_ref
from tests import f16x1_ref as R
from tests import gn_ref
from tests import test_gpu_gn_partials as G
from tests import test_gpu_wide_conv as T

pytestmark = pytest.mark.gpu

UNSPLIT = (4, 10, 12, 24)
# worst err(id) / err(tile) on the narrow shapes at 16 x 16 (tools/wide_plane_accuracy.py prints them; profiles/wide_plane_accuracy.txt)
R_PLANE = {10: 1.166, 12: 0.763, 4: 1.130}
NARROW = [(672, 288, 16), (384, 384, 16)]

CASES = [
    # (id, B, C0, C1, Cout, H)
    (10, 2, 1040, 0, 32, 16),       # the first 16 entries of the third slot, 65 chunks
    (10, 1, 2048, 0, 32, 16),       # the cap, all four slots full
    (10, 2, 768, 576, 96, 16),      # the concat seam, cout tile 3
    (10, 1, 1530, 0, 32, 16),       # CinP 1536, the clamped source of a padded last chunk
    (10, 1, 1152, 0, 64, 32),       # 32 x 32, regions with halos on all sides
    (12, 2, 1152, 0, 96, 16),       # two pieces
    (12, 1, 2048, 0, 32, 32),
    (24, 2, 1344, 0, 96, 16),       # one piece
    (24, 1, 2048, 0, 32, 16),
    (4, 2, 1152, 0, 64, 16),        # fp32, the second entry of a thread
    (4, 1, 2048, 0, 32, 32),
]


@pytest.fixture(scope="module")
def ctx():
    from tests.hiputil import Ctx
    return Ctx()


@pytest.mark.parametrize("shape,B,C0,C1,Cout,H", CASES, ids=lambda v: str(v))
def test_forced_wide_plane_layer_runs_its_unsplit_id_and_meets_its_gates(ctx, shape, B, C0, C1, Cout, H):
    for e in T._errors(ctx, shape, B, C0, C1, Cout, H):
        pro, got, err = e["pro"], e["got"], e["err"]
        worst, scale, mag = err.max().item(), e["scale"], e["mag"]
        assert e["ran"] == shape, f"forced {shape} at {C0}+{C1} channels, ran {e['ran']}"
        assert torch.isfinite(got).all()
        assert torch.equal(got, e["again"]), f"pro {pro}: two runs differ"
        if shape == 24:
            _, bound = R.wino_f16x1(e["d"], e["w"])
            bound = bound + 2.0 ** -23 * e["bias"].double().abs().reshape(1, -1, 1, 1)
            ratio = (err / bound).max().item()
            print(f"id {shape} B{B} {C0}+{C1}->{Cout} @{H} pro {pro}: worst |err| / bound {ratio:.4f}, max|err| / max|y| {worst / scale:.2e}")
            assert (err <= bound).all(), f"pro {pro}: |err| / bound = {ratio:.3f}"
            assert worst > 1e-5 * scale, "fp32-sized error: one fp16 piece did not run"
            continue
        norm, floor = (scale, 1e-6) if shape in T.TWO_PIECE else (mag, 2e-7)
        print(f"id {shape} B{B} {C0}+{C1}->{Cout} @{H} pro {pro}: err / norm {worst / norm:.3e}, tile {e['err_tile'] / norm:.3e}, "
              f"ratio {worst / e['err_tile']:.3f} (r narrow {R_PLANE[shape]}), max|err| / max|y| {worst / scale:.2e}")
        assert worst <= 1e-4 * scale + 2e-5 * max(scale, 1.0), f"pro {pro}: max-abs err {worst:.3e} (scale {scale:.3e})"
        assert worst / norm <= max(2.0 * R_PLANE[shape] * e["err_tile"] / norm, floor), \
            f"pro {pro}: err {worst / norm:.3e} vs tile {e['err_tile'] / norm:.3e}, r {R_PLANE[shape]}"


@pytest.mark.parametrize("shape,Cin", [(10, 2064), (11, 2304)], ids=["10@2064", "11@2304"])
def test_refused_plane_launches_end_on_a_direct_tile(ctx, shape, Cin):
    """16 x 16: an unsplit launch above WINO_TABLE_CH_PLANE channels, and the 2-way split above WINO_MAX_CIN (its part of 1152 channels would fit
    the table: the channel bound refuses it).  Every id of the fallback list refuses, and the launch ends on a direct tile with the right result."""
    x, w, bias, coef = T._case(1, Cin, 0, 32, 16)
    got, ran = T._run(ctx, shape, x.cuda(), None, w.cuda(), bias.cuda(), dict(coef=coef.cuda(), act=1))
    print(f"conv_shape {shape} at {Cin} channels, 16 x 16, ran {ran}")
    assert 0 <= ran <= 3, ran
    y64 = F.conv2d(R.activate(x, coef, True), w.double(), bias.double(), padding=1)
    scale = y64.abs().max().item()
    assert (got.cpu().double() - y64).abs().max().item() <= 1e-4 * scale + 2e-5 * max(scale, 1.0)


@pytest.mark.parametrize("kid", UNSPLIT)
def test_unsplit_epilogue_partials_at_1152_channels(ctx, kid):
    """The GroupNorm partials come out of the unsplit epilogue as for every narrower layer: np = (H / 8)(W / 16), within the bounds
    tests/test_gpu_gn_partials.py holds every producer to (tests/gn_ref.py)."""
    H = 16
    r = G.measure(ctx, G._c(kid, 1, 1152, 0, 40, H))
    print({k: v for k, v in r.items() if k not in ("y", "A")})
    assert r["ran"] == kid, f"kernel {r['ran']} ran, {kid} was asked for"
    assert r["np"] == (H // 8) * (H // 16) == gn_ref.expected_np(kid, H, H, 1), r["np"]
    assert r["written_finite"] and r["rest_untouched"] and r["repeatable"]
    assert r["sum_ratio"] <= 1.0, f"folded sum off by {r['sum_ratio']:.3g} x the gate"
    assert r["m2_err"] <= 1e-4 * r["m2_max"], f"folded M2 off by {r['m2_err']:.3e}, largest M2 {r['m2_max']:.3e}"
    assert r["coef_ratio0"] <= 1.0 and r["coef_ratio1"] <= 1.0, (r["coef_ratio0"], r["coef_ratio1"])


# ------------------------------------------------------------------------------------------------ a model
def _config():
    """Two levels of the ngf-288 widths, 576 / 864 at 32 x 32 / 16 x 16: the up path concatenates 864 + 864 and 864 + 576 at 16 x 16 and
    864 + 576 at 32 x 32 (then 576 + 288 = 864, below the line)."""
    config = synth.make_config("tiny")
    config.data.image_size = 32
    config.model.ngf = 288
    config.model.n_head_channels = 288
    config.model.ch_mult = [2, 3]
    config.model.num_res_blocks = 1
    config.model.attn_resolutions = [16]
    config.device = "cuda:0"
    return config


def _planned_wide3(config):
    """[(H, Cin, Cout)] of the 3x3 convs above 1024 input channels, from the module plan: Conv_0 of a res block reads its cin (behind the
    block's resampling, if any), Conv_1 its cout."""
    c = unet_ref.hot_cfg(config)
    H, out = c.image_size, []
    for m in unet_ref.module_plan(c):
        if m["kind"] != "res":
            continue
        H = H // 2 if m["down"] else H * 2 if m["up"] else H
        out += [(H, cin, m["cout"]) for cin in (m["cin"], m["cout"]) if cin > 1024]
    return sorted(out)


def test_model_runs_its_32x32_layer_above_1024_channels_on_an_unsplit_winograd_kernel():
    from mcvd_pytorch_amd.scorenet import HipScoreNet
    config = _config()
    assert _planned_wide3(config) == [(16, 1440, 864), (16, 1728, 864), (32, 1440, 576)]
    sd = synth.make_state_dict(config, seed=123)
    net = HipScoreNet(config)
    net.load_state_dict(sd, strict=True)
    net.eval()
    x, cond = synth.make_inputs(config, 1, seed=0)
    t = torch.tensor([470])
    torch.set_num_threads(16)
    with torch.no_grad():
        ref = unet_ref.unet_forward(sd, config, x, t, cond)
    x, t, cond = x.cuda(), t.cuda(), cond.cuda()
    eps = net(x, t, cond=cond).clone()                      # the autotuned forward
    scale = ref.abs().max().item()
    err = (eps.cpu() - ref).abs().max().item()
    wide = T._wide3(T._conv_ops(net))
    print(f"|eps - reference| {err:.3e} of max {scale:.3f}; 3x3 convs above 1024 channels (H, Cin, Cout, kernel):", [(o[2], o[3], o[4], o[5]) for o in wide])
    assert err <= 1e-4 * scale
    assert sorted((o[2], o[3], o[4]) for o in wide) == _planned_wide3(config), wide
    assert all(o[5] in T.WINO_IDS for o in wide), wide
    assert all(o[5] in (10, 4) for o in wide if o[2] == 32), wide          # no K-split scratch above 16 x 16: unsplit, or the tile (the parent)
    net.set_option("graph", 1)                              # eager, captured, replayed
    try:
        for _ in range(3):
            assert torch.equal(net(x, t, cond=cond), eps)
    finally:
        net.set_option("graph", 0)
    net.set_option("f16x2", 1)
    try:
        a = net(x, t, cond=cond).clone()
        wide2 = T._wide3(T._conv_ops(net))
    finally:
        net.set_option("f16x2", 0)
    print("under f16x2:", [(o[2], o[3], o[4], o[5]) for o in wide2])
    assert len(wide2) == 3 and all(o[6] for o in wide2), wide2              # (each of them sits behind a GroupNorm)
    assert all(o[5] in T.TWO_PIECE for o in wide2), wide2
    assert (a - eps).abs().max().item() <= 2e-5 * eps.abs().max().item()          # the gate of tests/test_gpu_wide_conv.py
    assert (a.cpu() - ref).abs().max().item() <= 1e-4 * scale
