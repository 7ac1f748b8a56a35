"""GPU: LPIPS on the device -- mcvd_lpips_* (kernels/lpips.cpp) and mcvd_op_conv2d_strided (the detector nets' one conv,
kernels/detector_ops.cpp) through the C ABI -- against tests/lpips_ref.py
(the integer resize and the fp64 restatement) and against what the REAL PerceptualLoss / NCSNRunner.video_gen computed over the seeded
backbone (fixtures lpips_direct.pt, lpips_runner_*.pt; cases in tests/test_lpips_cpu.py).

Gates:
  * resized planes: exact (integer arithmetic, Pillow's tables);
  * device values (frame, per tap, tap tensors): relative deviation from the fp64 restatement <= GATE_FACTOR = 8 x the fixture's
    ref_rel_dev, the real reference's own fp32 result measured against fp64 when the fixture was made (1.2e-7 ... 2.0e-7), never a figure
    of the code under test.  Both are fp32 roundings of the same sums (K up to 3 456) in different orders; single layers here are held
    to 1.5 x, and five stacked layers, a division by a norm and a difference of near-equal unit vectors compound that.  For a tap TENSOR
    the relative deviation is the 2-norm of the difference over the 2-norm of the fp64 tensor.  The summary keys are host arithmetic on
    the frame values and are held to the same relative gate (conf95 = 1.96 sem moves by at most twice the per-video bound);
  * mcvd_op_conv2d_strided against F.conv2d in fp64: |y - y64| <= min((K + 2) 2^-24, 2e-6) x conv(|x|, |w|) + |bias| per element -- the
    fp32 bound of a K-term fma chain plus the bias add and the final rounding, capped by the 2e-6 this repository holds its other fp32
    convs to (test_conv_bf16x3_is_fp32_accurate);
  * mcvd_op_conv2d_strided against mcvd_op_conv2d_rect without alpha: equal (one kernel; a bias add is its fma epilogue with alpha absent).
Measured ratios are printed by every test.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import synth
from tests import lpips_ref
from tests.hiputil import Ctx, P
from tests.test_lpips_cpu import RUNNER_CASES, direct, runner
from tests.test_video_metrics_cpu import fixture

pytestmark = pytest.mark.gpu

GATE_FACTOR = 8
EINVAL, ESTATE = -1, -3


def _net(g):
    from mcvd_pytorch_amd import LpipsNet
    net = LpipsNet(device="cuda:0")
    net.load_backbone(lpips_ref.make_backbone(g["seed"]))
    net.load_linear({f"lin{k}.model.1.weight": g["lins"][k].reshape(1, -1, 1, 1) for k in range(5)})
    net.load_state_dict({"scaling_layer.shift": g["shift"].reshape(1, 3, 1, 1), "scaling_layer.scale": g["scale"].reshape(1, 3, 1, 1)})
    return net


def _ref(g, pred, real, Cc):
    return lpips_ref.frame_lpips64(pred, real, Cc, lpips_ref.make_backbone(g["seed"]), g["lins"], g["shift"], g["scale"])


def _rel(got, want):
    got, want = got.double().cpu().reshape(-1), want.reshape(-1)
    zero = want == 0
    assert torch.equal(got[zero], want[zero]), "an exactly-zero distance is not exactly zero on the device"
    return ((got[~zero] - want[~zero]).abs() / want[~zero]).max().item() if (~zero).any() else 0.0


def test_every_frame_of_the_direct_fixture(golden_dir):
    """Resized planes equal to Pillow's, every byte; every frame value and per-tap value within 8 x ref_rel_dev of the fp64 restatement;
    the identical pair exactly 0.0."""
    from mcvd_pytorch_amd import frame_lpips
    g = direct(golden_dir)
    net = _net(g)
    gate = GATE_FACTOR * g["ref_rel_dev"]
    worst = 0.0
    for c in g["cases"]:
        name, Cc = c["name"], c["channels"]
        fr = g[f"frames_{name}"]
        val, taps, planes = frame_lpips(fr[0].cuda(), fr[1].cuda(), Cc, net, return_taps=True)
        assert val.dtype == torch.float32 and tuple(val.shape) == (c["B"], c["T"])
        assert torch.equal(planes.cpu(), g[f"resized_{name}"]), name
        v64, pt64, _ = _ref(g, fr[0], fr[1], Cc)
        dv, dt = _rel(val, v64), _rel(taps, pt64)
        worst = max(worst, dv, dt)
        print(f"  {name}: frame {dv:.3e} per-tap {dt:.3e} -> ratio to ref_rel_dev {max(dv, dt) / g['ref_rel_dev']:.2f} (gate {GATE_FACTOR})")
        assert dv <= gate and dt <= gate, name
        if name == "c3_32_identical":
            assert val[0, 1].item() == 0.0 and val[0, 0].item() > 0
    print(f"  lpips_direct: worst ratio {worst / g['ref_rel_dev']:.2f}")


SHAPES = [(4, 3, 128, 128, 64, 11, 4, 2), (4, 64, 15, 15, 192, 5, 1, 2), (6, 192, 7, 7, 384, 3, 1, 1), (6, 384, 7, 7, 256, 3, 1, 1),
          (6, 256, 7, 7, 256, 3, 1, 1), (2, 5, 37, 29, 70, 7, 3, 2), (3, 17, 20, 33, 33, 1, 2, 0), (1, 8, 9, 9, 8, 3, 1, 1), (5, 6, 11, 13, 100, 5, 2, 4),
          (1, 2, 20, 20, 8, 17, 1, 8)]      # the last: 17 taps per side, beyond the 4 bits a tap once had in the conv's table
IDS = ["alex1", "alex2", "alex3", "alex4", "alex5", "k7s3", "k1s2", "b1", "k5s2p4", "k17"]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_conv2d_strided_against_fp64(shape):
    B, Cin, H, W, Cout, ks, stride, pad = shape
    from mcvd_pytorch_amd import _lib
    ctx = Ctx()
    gen = torch.Generator().manual_seed(Cin * 100 + ks)
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, ks, ks, generator=gen) / (Cin * ks * ks) ** 0.5
    bias = 0.1 * torch.randn(Cout, generator=gen)
    K = Cin * ks * ks
    for relu, b in ((0, bias), (1, bias), (0, None)):
        want = F.conv2d(x.double(), w.double(), None if b is None else b.double(), stride=stride, padding=pad)
        if relu:
            want = want.relu()
        mag = F.conv2d(x.double().abs(), w.double().abs(), None if b is None else b.double().abs(), stride=stride, padding=pad)
        y = torch.full(want.shape, float("nan"), device="cuda")
        xc, wc, bc = x.cuda(), w.cuda(), None if b is None else b.cuda()
        _lib.check(_lib.lib.mcvd_op_conv2d_strided(ctx.h, P(xc), P(wc), P(bc), B, Cin, H, W, Cout, ks, stride, pad, relu, P(y)), "conv2d_strided")
        err = ((y.cpu().double() - want).abs() / mag).max().item()
        bound = min((K + 2) * 2.0 ** -24, 2e-6)
        print(f"  conv {shape} relu {relu} bias {b is not None}: max err / conv(|x|,|w|) {err:.3e} (bound {bound:.3e})")
        assert torch.isfinite(y).all() and err <= bound


@pytest.mark.parametrize("name", ["b1", "k1s2", "alex1"])
def test_conv2d_strided_is_conv2d_rect_without_alpha(name):
    """The two ops are one kernel: op_conv2d_strided(x, w, bias, relu) equals op_conv2d_rect(x, w, alpha=None, beta=bias, kh = kw = ks,
    ph = pw = pad, relu, c0 = 0, Ctot = Cout) -- a bias add is the fma epilogue with alpha absent.  b1: one image, less than one tile in
    every dimension; k1s2: a 1 x 1 kernel that must not take the plain-load path; alex1: 11 taps per side."""
    B, Cin, H, W, Cout, ks, stride, pad = SHAPES[IDS.index(name)]
    from mcvd_pytorch_amd import _lib
    ctx = Ctx()
    gen = torch.Generator().manual_seed(Cin * 100 + ks)
    x = torch.randn(B, Cin, H, W, generator=gen).cuda()
    w = (torch.randn(Cout, Cin, ks, ks, generator=gen) / (Cin * ks * ks) ** 0.5).cuda()
    bias = (0.1 * torch.randn(Cout, generator=gen)).cuda()
    OH, OW = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    for relu in (0, 1):
        a = torch.full((B, Cout, OH, OW), float("nan"), device="cuda")
        b = torch.full((B, Cout, OH, OW), float("nan"), device="cuda")
        _lib.check(_lib.lib.mcvd_op_conv2d_strided(ctx.h, P(x), P(w), P(bias), B, Cin, H, W, Cout, ks, stride, pad, relu, P(a)), "conv2d_strided")
        _lib.check(_lib.lib.mcvd_op_conv2d_rect(ctx.h, P(x), P(w), None, P(bias), B, Cin, H, W, Cout, ks, ks, stride, pad, pad, relu, P(b), 0, Cout),
                   "conv2d_rect")
        assert torch.isfinite(a).all() and torch.equal(a, b), (name, relu)


def test_tap_tensors_of_the_two_stored_images(golden_dir):
    """The AlexNet chain through mcvd_op_conv2d_strided (the kernel the net runs) on the two stored images: each tap within
    8 x ref_rel_dev (2-norm) of the fp64 restatement, and as close to the real net's stored fp32 taps as that implies."""
    from mcvd_pytorch_amd import _lib
    g = direct(golden_dir)
    bb = lpips_ref.make_backbone(g["seed"])
    ctx = Ctx()
    gate = GATE_FACTOR * g["ref_rel_dev"]
    for ti, (cn, which, b, t) in enumerate(g["tap_images"]):
        x = lpips_ref.net_input(g[f"resized_{cn}"][which, b, t][None])
        want = lpips_ref.taps(x, bb, g["shift"], g["scale"])
        h = ((x - g["shift"].reshape(1, 3, 1, 1)) / g["scale"].reshape(1, 3, 1, 1)).cuda()
        for k, ((idx, _, cout, cin, ks, stride, pad), pool) in enumerate(zip(lpips_ref.CONVS, lpips_ref.POOL_BEFORE)):
            if pool:
                h = F.max_pool2d(h, 3, 2).contiguous()
            oh = (h.shape[2] + 2 * pad - ks) // stride + 1
            y = torch.empty(1, cout, oh, oh, device="cuda")
            wt, bs = bb[f"features.{idx}.weight"].cuda(), bb[f"features.{idx}.bias"].cuda()
            _lib.check(_lib.lib.mcvd_op_conv2d_strided(ctx.h, P(h), P(wt), P(bs), 1, cin, h.shape[2], h.shape[3], cout, ks, stride, pad, 1, P(y)))
            d = ((y.cpu().double() - want[k]).norm() / want[k].norm()).item()
            dr = ((g[f"tap{k + 1}_real"][ti].double() - want[k][0]).norm() / want[k].norm()).item()
            print(f"  image {ti} tap {k + 1}: device {d:.3e}, real net {dr:.3e}, ratio to ref_rel_dev {d / g['ref_rel_dev']:.2f}")
            assert d <= gate
            h = y


@pytest.mark.parametrize("case", RUNNER_CASES)
def test_against_the_real_runner(golden_dir, case):
    """The frames of the real video_gen run through VideoMetrics(..., lpips=net): every frame value within 8 x ref_rel_dev of the fp64
    restatement, vid_lpips and the lpips keys of the real runner's vid_metrics within the same relative gate (conf95: twice), the other
    keys as without LPIPS, and the key set the real runner's (without ckpt)."""
    from mcvd_pytorch_amd import VideoMetrics, frame_lpips
    g, fx = runner(golden_dir, case), fixture(golden_dir, case)
    net = _net(g)
    cfg = synth.make_config(g["config_name"])
    cfg.data.dataset = g["dataset"]
    Cc = g["channels"]
    gate = GATE_FACTOR * g["ref_rel_dev"]
    vm = VideoMetrics(cfg, preds_per_test=g["preds_per_test"], lpips=net)
    plain = VideoMetrics(cfg, preds_per_test=g["preds_per_test"])
    worst = 0.0
    for ph in (1, 2):
        for bi, (pred, real) in enumerate(fx["frames"][ph]):
            vm.update(pred.cuda(), real.cuda(), phase=ph)
            plain.update(pred.cuda(), real.cuda(), phase=ph)
            val = frame_lpips(pred.cuda(), real[:, :pred.shape[1]].cuda(), Cc, net)
            d = _rel(val, g["value64"][ph][bi])
            dr = _rel(val, g["value"][ph][bi].double())
            worst = max(worst, d)
            print(f"  {case} phase {ph} batch {bi}: vs fp64 {d:.3e} (ratio {d / g['ref_rel_dev']:.2f}, gate {GATE_FACTOR}), vs the real runner's fp32 {dr:.3e}")
            assert d <= gate
    got, want, base = vm.summary(), g["vid_metrics"], plain.summary()
    assert set(got) == {k for k in want if k != "ckpt"} and set(base) == {k for k in got if "lpips" not in k}
    for k, v in base.items():
        assert got[k] == v or (math.isnan(got[k]) and math.isnan(v)), k
    for ph, key in ((1, "vid_lpips"), (2, "vid_lpips2")):
        if g[key] is None:
            assert not vm.vid_lpips[ph]
            continue
        a, b = np.array(vm.vid_lpips[ph]), np.array(g[key])
        assert a.shape == b.shape and np.all(np.abs(a - b) <= 2 * gate * b)      # both sides are within `gate` of the fp64 value
    for k in got:
        if "lpips" not in k:
            continue
        scale = max(g["vid_lpips2" if "lpips2" in k else "vid_lpips"])      # every per-video value moves by at most gate x itself
        f = 2 * (2 if k.endswith("_conf95") else 1)
        if math.isnan(want[k]):
            assert math.isnan(got[k])
        else:
            assert abs(got[k] - want[k]) <= f * gate * scale, (k, got[k], want[k])
    print(f"  lpips_runner_{case}: worst ratio {worst / g['ref_rel_dev']:.2f}")


def test_deterministic_and_independent_of_the_chunking(golden_dir):
    """Two calls give identical bits; B * T = 150 frames (three chunks of 64, 64, 22) equal the same frames sent in calls of 64, 64, 22 and
    in calls of 1 x 150 rows, bit for bit; nothing NaN."""
    from mcvd_pytorch_amd import frame_lpips
    g = direct(golden_dir)
    net = _net(g)
    gen = torch.Generator().manual_seed(3)
    real = torch.rand(150, 1, 32, 32, generator=gen)
    pred = (real + 0.1 * torch.randn(150, 1, 32, 32, generator=gen)).clamp(0, 1)
    p, r = pred.cuda(), real.cuda()
    a, ta, pa = frame_lpips(p, r, 1, net, return_taps=True)
    b, tb, pb = frame_lpips(p, r, 1, net, return_taps=True)
    assert torch.equal(a, b) and torch.equal(ta, tb) and torch.equal(pa, pb) and torch.isfinite(a).all() and (a > 0).all()
    parts = torch.cat([frame_lpips(p[i:j], r[i:j], 1, net) for i, j in ((0, 64), (64, 128), (128, 150))])
    assert torch.equal(parts, a)
    as_frames = frame_lpips(p.reshape(1, 150, 32, 32), r.reshape(1, 150, 32, 32), 1, net)
    assert torch.equal(as_frames.reshape(-1), a.reshape(-1))
    v64, _, _ = _ref(g, pred[:8], real[:8], 1)
    assert _rel(a[:8], v64) <= GATE_FACTOR * g["ref_rel_dev"]


def test_errors(golden_dir):
    """Missing weights -> MCVD_ESTATE naming the tensor; frames before finalize -> MCVD_ESTATE; C = 2 -> MCVD_EINVAL; unknown name and
    wrong size -> MCVD_EINVAL; Python raises for them."""
    from mcvd_pytorch_amd import LpipsNet, _lib, frame_lpips
    g = direct(golden_dir)
    lib = _lib.lib
    ctx = Ctx()
    h = C.c_void_p()
    assert lib.mcvd_lpips_create(ctx.h, C.byref(h)) == 0
    assert lib.mcvd_lpips_finalize(h) == ESTATE and "net.slice1.0.weight" in _lib.last_error()
    bb = lpips_ref.make_backbone(g["seed"])

    def put(name, t):
        t = t.contiguous().float()
        return lib.mcvd_lpips_set_param(h, name.encode(), P(t), (C.c_int64 * t.dim())(*t.shape), t.dim(), 1 if t.is_cuda else 0)
    for k, v in bb.items():
        assert put(k, v.cuda() if "bias" in k else v) == 0      # biases from the device, weights from the host
    assert lib.mcvd_lpips_finalize(h) == ESTATE and "lin0.model.1.weight" in _lib.last_error()
    assert put("lin9.model.1.weight", g["lins"][0]) == EINVAL and put("lin0.model.1.weight", g["lins"][1]) == EINVAL
    x = torch.rand(1, 3, 32, 32, device="cuda")
    out = torch.empty(1, device="cuda")
    assert lib.mcvd_lpips_frames(h, P(x), P(x), 1, 1, 3, 32, 32, P(out), None, None) == ESTATE
    for k in range(5):
        assert put(f"lin{k}.model.1.weight", g["lins"][k].reshape(1, -1, 1, 1)) == 0
    assert lib.mcvd_lpips_finalize(h) == ESTATE and "scaling_layer.shift" in _lib.last_error()
    assert put("scaling_layer.shift", g["shift"]) == 0 and put("scaling_layer.scale", g["scale"]) == 0
    assert lib.mcvd_lpips_finalize(h) == 0
    x2 = torch.rand(1, 2, 32, 32, device="cuda")
    assert lib.mcvd_lpips_frames(h, P(x2), P(x2), 1, 1, 2, 32, 32, P(out), None, None) == EINVAL
    assert lib.mcvd_lpips_frames(h, None, P(x), 1, 1, 3, 32, 32, P(out), None, None) == EINVAL
    assert lib.mcvd_lpips_frames(h, P(x), P(x), 1, 1, 3, 32, 32, None, None, None) == EINVAL
    assert lib.mcvd_lpips_frames(h, P(x), P(x), 1, 1, 3, 32, 32, P(out), None, None) == 0
    torch.cuda.synchronize()
    assert out.item() == 0.0
    want = frame_lpips(x, x.flip(-1).contiguous(), 3, _net(g))
    assert lib.mcvd_lpips_frames(h, P(x), P(x.flip(-1).contiguous()), 1, 1, 3, 32, 32, P(out), None, None) == 0
    torch.cuda.synchronize()
    assert out.item() == want.item() > 0
    lib.mcvd_lpips_destroy(h)
    empty = LpipsNet(device="cuda:0")
    with pytest.raises(RuntimeError, match="missing"):
        frame_lpips(x, x, 3, empty)
    with pytest.raises(ValueError):
        frame_lpips(x2, x2, 2, empty)


def test_on_a_scorenets_context_and_beyond_the_data(golden_dir):
    """LpipsNet(scorenet=net) runs on the net's context and gives the same bits; 'cannot calculate' appends zeros to vid_lpips too."""
    from mcvd_pytorch_amd import HipScoreNet, LpipsNet, VideoMetrics, frame_lpips
    g = direct(golden_dir)
    cfg = synth.make_config("tiny")
    cfg.device = "cuda:0"
    sn = HipScoreNet(cfg)
    a = _net(g)
    b = LpipsNet(scorenet=sn)
    b.load_backbone(lpips_ref.make_backbone(g["seed"])).load_linear({f"lin{k}.model.1.weight": g["lins"][k] for k in range(5)})
    fr = g["frames_c1_64"]
    assert torch.equal(frame_lpips(fr[0].cuda(), fr[1].cuda(), 1, a), frame_lpips(fr[0].cuda(), fr[1].cuda(), 1, b))
    assert torch.equal(g["shift"], torch.tensor([-.030, -.088, -.188])) and torch.equal(g["scale"], torch.tensor([.458, .448, .450]))
    vm = VideoMetrics(cfg, lpips=a)
    vm.update(fr[0].cuda(), fr[1][:, :1].cuda())
    assert vm.vid_lpips[1] == [0, 0] and vm.summary() is None
