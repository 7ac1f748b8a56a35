"""GPU: video_gen's test-mode metrics on the device -- mcvd_frame_metrics (kernels/metrics.cpp) through frame_metrics / VideoMetrics --
against tests/metrics_ref.py (the CPU restatement; no scipy or PIL needed) and against what the REAL `NCSNRunner.video_gen` computed
(fixtures tests/golden/video_metrics_*.pt, tools/gen_video_metrics_golden.py; cases listed in tests/test_video_metrics_cpu.py).

Gates:
  * grey planes (quantisation x.mul(255).byte(), the MNIST rule's round, Pillow's integer luma): exact -- one IEEE multiply and
    truncation, then integer arithmetic;
  * per-frame SSIM vs the restatement (both fp64): 1e-9.  The moments are <= 255^2 = 65025; 22 fp64 taps err by <= 22 * 65025 * 2^-53
    ~ 1.6e-10 absolute, doubled by the variance cancellation; the denominators are >= C1 = 6.5 and >= C2 = 58.5, so S moves by ~1e-11;
  * per-frame MSE vs the fp64 mean of the fp32 differences: 1 fp32 ulp (fp64 accumulation of <= 49 152 terms errs by ~6e-12 relative);
    per-video MSE vs the real runner's fp32 value: 3 x the recorded distance between that value and its fp64 counterpart, floored at
    1 ulp (the project's rule for loosened gates).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import synth
from tests import metrics_ref
from tests.test_video_metrics_cpu import CASES, fixture

pytestmark = pytest.mark.gpu

SSIM_TOL = 1e-9
LOG10E10 = 10.0 / math.log(10.0)


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def _inputs(B, T, Cc, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    real = torch.rand(B, T * Cc, H, W, generator=g)
    pred = (real + 0.2 * torch.randn(B, T * Cc, H, W, generator=g)).clamp(0.0, 1.0)
    return pred, real


def _check_frames(pred, real, Cc, binary):
    """The device's per-frame values against the restatement: SSIM 1e-9, MSE 1 fp32 ulp of the fp64 mean."""
    from mcvd_pytorch_amd import frame_metrics
    mse, ssim = frame_metrics(pred.cuda(), real.cuda(), Cc, binary=binary)
    mse, ssim = mse.cpu(), ssim.cpu()
    assert mse.dtype == torch.float32 and ssim.dtype == torch.float64
    gp, gr = metrics_ref.grey_planes(pred, Cc, binary), metrics_ref.grey_planes(real, Cc, binary)
    B, T, H, W = gp.shape
    want_s = metrics_ref.ssim_planes(gp.reshape(B * T, H, W), gr.reshape(B * T, H, W)).reshape(B, T)
    want_m = metrics_ref.frame_mse64(pred, real, Cc)
    ds = (ssim - want_s).abs().max().item()
    dm = np.abs(mse.double().numpy() - want_m.numpy())
    print(f"  [{B}, {T}, {Cc}, {H}, {W}] binary {binary}: max |dSSIM| {ds:.3e}, max |dMSE| / ulp {(dm / _ulp32(want_m.numpy())).max():.3f}")
    assert ds <= SSIM_TOL
    assert np.all(dm <= _ulp32(want_m.numpy()))
    return mse, ssim


def test_quantisation_is_exact():
    """x = fp32(k / 255), k = 0..255, and both fp32 neighbours of each, as one C = 1 frame: the grey plane equals torch's x.mul(255).byte(),
    and x.round().mul(255).byte() under the MNIST rule."""
    from mcvd_pytorch_amd import frame_metrics
    x = torch.arange(256, dtype=torch.float32) / 255
    x = torch.stack([torch.nextafter(x, torch.tensor(-1.0)), x, torch.nextafter(x, torch.tensor(2.0))], dim=1).reshape(1, 1, 24, 32)
    for binary in (False, True):
        _, _, grey = frame_metrics(x.cuda(), x.flip(-1).contiguous().cuda(), 1, binary=binary, return_grey=True)
        want = (x.round() if binary else x).mul(255).byte()
        assert torch.equal(grey[0, 0].cpu(), want[:, 0]) and torch.equal(grey[1, 0].cpu(), want[:, 0].flip(-1))


def test_luma_is_exact_on_every_rgb_triple():
    """All 2^24 RGB triples as one 3-channel 4096 x 4096 frame, values (k + 0.5) / 255: the grey plane equals Pillow's integer formula."""
    from mcvd_pytorch_amd import frame_metrics
    k = torch.arange(1 << 24, dtype=torch.int64)
    rgb = torch.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255]).reshape(1, 3, 4096, 4096)
    x = ((rgb.float() + 0.5) / 255).cuda()
    _, _, grey = frame_metrics(x, x, 3, return_grey=True)
    want = metrics_ref.luma(rgb[0, 0], rgb[0, 1], rgb[0, 2]).to(torch.uint8)
    assert torch.equal(grey[0, 0, 0].cpu(), want) and torch.equal(grey[1, 0, 0].cpu(), want)


@pytest.mark.parametrize("shape", [(64, 20, 1, 64, 64, True), (8, 28, 3, 128, 128, False), (3, 2, 1, 11, 12, False),
                                   (2, 3, 3, 11, 12, True), (2, 2, 3, 37, 70, False)],
                         ids=["config2_mnist", "config5", "11x12", "11x12_rgb_mnist", "37x70"])
def test_per_frame_values_against_the_restatement(shape):
    B, T, Cc, H, W, binary = shape
    pred, real = _inputs(B, T, Cc, H, W, seed=B * 1000 + H)
    _check_frames(pred, real, Cc, binary)


@pytest.mark.parametrize("case", [c for c in CASES if c != "beyond"])
def test_per_frame_values_on_the_fixture_frames(golden_dir, case):
    """The same gates on the frames the real runner's metric loop saw (the 'beyond' case has none: its real clips are too short)."""
    g = fixture(golden_dir, case)
    Cc = g["channels"]
    for ph in (1, 2):
        for pred, real in g["frames"][ph]:
            _check_frames(pred, real[:, :pred.shape[1]], Cc, g["dataset"].upper() in metrics_ref.MNIST)


def test_identical_frames():
    """pred == real: mse 0, psnr inf, ssim within 1e-9 of 1."""
    from mcvd_pytorch_amd import VideoMetrics
    _, real = _inputs(2, 3, 3, 11, 12, seed=4)
    mse, ssim = _check_frames(real, real, 3, False)
    assert torch.all(mse == 0) and (ssim - 1).abs().max().item() <= SSIM_TOL
    cfg = synth.make_config("tiny")
    cfg.data.channels = 3
    vm = VideoMetrics(cfg)
    vm.update(real, real)
    s = vm.summary()
    assert s["mse"] == 0.0 and s["psnr"] == math.inf and abs(s["ssim"] - 1) <= SSIM_TOL


def test_deterministic():
    from mcvd_pytorch_amd import frame_metrics
    pred, real = _inputs(8, 28, 3, 128, 128, seed=9)
    p, r = pred.cuda(), real.cuda()
    a = frame_metrics(p, r, 3)
    b = frame_metrics(p, r, 3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_errors():
    """C = 2 and H = 10 raise ValueError in Python; the C ABI returns MCVD_EINVAL for them and for NULL required pointers."""
    from mcvd_pytorch_amd import _lib, frame_metrics
    from mcvd_pytorch_amd.metrics import _package_ctx
    with pytest.raises(ValueError):
        frame_metrics(torch.zeros(1, 2, 16, 16).cuda(), torch.zeros(1, 2, 16, 16).cuda(), 2)
    with pytest.raises(ValueError):
        frame_metrics(torch.zeros(1, 1, 10, 16).cuda(), torch.zeros(1, 1, 10, 16).cuda(), 1)
    ctx = _package_ctx(torch.device("cuda", 0))
    x = torch.zeros(1, 3, 16, 16, device="cuda")
    mse = torch.empty(1, device="cuda")
    ssim = torch.empty(1, dtype=torch.float64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    EINVAL = -1
    assert _lib.lib.mcvd_frame_metrics(ctx, ptr(x), ptr(x), 1, 1, 2, 16, 16, 0, ptr(mse), ptr(ssim), None) == EINVAL
    assert _lib.lib.mcvd_frame_metrics(ctx, ptr(x), ptr(x), 1, 1, 3, 10, 16, 0, ptr(mse), ptr(ssim), None) == EINVAL
    assert _lib.lib.mcvd_frame_metrics(ctx, ptr(x), ptr(x), 1, 1, 3, 16, 10, 0, ptr(mse), ptr(ssim), None) == EINVAL
    assert _lib.lib.mcvd_frame_metrics(ctx, None, ptr(x), 1, 1, 3, 16, 16, 0, ptr(mse), ptr(ssim), None) == EINVAL
    assert _lib.lib.mcvd_frame_metrics(ctx, ptr(x), None, 1, 1, 3, 16, 16, 0, ptr(mse), ptr(ssim), None) == EINVAL
    assert _lib.lib.mcvd_frame_metrics(ctx, ptr(x), ptr(x), 1, 1, 3, 16, 16, 0, None, ptr(ssim), None) == EINVAL
    assert _lib.lib.mcvd_frame_metrics(ctx, ptr(x), ptr(x), 1, 1, 3, 16, 16, 0, ptr(mse), None, None) == EINVAL
    assert _lib.lib.mcvd_frame_metrics(None, ptr(x), ptr(x), 1, 1, 3, 16, 16, 0, ptr(mse), ptr(ssim), None) == EINVAL
    assert _lib.lib.mcvd_frame_metrics(ctx, ptr(x), ptr(x), 1, 1, 3, 16, 16, 0, ptr(mse), ptr(ssim), None) == 0


def test_package_context_does_not_mark_the_device_shared():
    """frame_metrics without a scorenet, in a process that holds a HipScoreNet: both contexts on torch's current stream, so neither
    reports mcvd_ctx_device_shared; with the scorenet the call runs on the net's own context and gives the same values."""
    from mcvd_pytorch_amd import HipScoreNet, _lib, frame_metrics
    from mcvd_pytorch_amd.metrics import _ctxs
    cfg = synth.make_config("tiny")
    cfg.device = "cuda:0"
    net = HipScoreNet(cfg)
    pred, real = _inputs(2, 2, 1, 32, 32, seed=3)
    a = frame_metrics(pred.cuda(), real.cuda(), 1)
    torch.cuda.synchronize()
    assert _lib.lib.mcvd_ctx_device_shared(net._ctx) == 0
    assert _lib.lib.mcvd_ctx_device_shared(_ctxs[0]) == 0
    b = frame_metrics(pred.cuda(), real.cuda(), 1, scorenet=net)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert _lib.lib.mcvd_ctx_device_shared(net._ctx) == 0


def _mse_gates(vid_mse, vid_mse64):
    """Per-video MSE gate: 3 x |fp32 value - fp64 value| recorded from the real runner, floored at 1 fp32 ulp."""
    ref = np.asarray(vid_mse, dtype=np.float32)
    return np.maximum(3 * np.abs(ref.astype(np.float64) - np.asarray(vid_mse64, dtype=np.float64)), _ulp32(ref))


def _check_summary(got, want, e_mse, min_mse, max_psnr, sfx=""):
    """Summary keys from per-video values that differ by at most e_mse (MSE) and SSIM_TOL (SSIM).  mean and min/max move by at most the
    per-video bound, std by at most it (1-Lipschitz), conf95 = 1.96 sem by at most 1.96 sqrt(n / (n - 1)) / sqrt(n) <= 2 times it.
    PSNR = 10 log10(1 / mse) moves by (10 / ln 10) e_mse / min_mse, plus the fp32 rounding of 1 / mse, log10 and the product (4 ulp of
    the largest PSNR); each key also carries fp64 rounding of its own (1e-12 relative)."""
    e_psnr = LOG10E10 * e_mse / min_mse + 4 * float(_ulp32(max_psnr))
    for name, e in (("mse", e_mse), ("psnr", e_psnr), ("ssim", SSIM_TOL)):
        for k, f in ((f"{name}{sfx}", 1), (f"{name}{sfx}_std", 1), (f"{name}{sfx}_conf95", 2)):
            a, b = got[k], want[k]
            if math.isnan(b) or math.isinf(b):
                assert (math.isnan(a) and math.isnan(b)) or a == b, (k, a, b)
                continue
            assert abs(a - b) <= f * e + 1e-12 * abs(b), (k, a, b, f * e)


@pytest.mark.parametrize("case", CASES)
def test_against_the_real_runner(golden_dir, case):
    """The recorded [0, 1] frames of every phase through VideoMetrics on the device: per-frame SSIM within 1e-9 of the real runner's, the
    grey planes equal to the real-Pillow planes, per-video MSE within 3 x the recorded fp32-vs-fp64 distance, and the summary within
    what those bounds allow (_check_summary); the 'beyond' case appends zeros and reports no summary, as the runner returns None."""
    from mcvd_pytorch_amd import VideoMetrics, frame_metrics
    g = fixture(golden_dir, case)
    cfg = synth.make_config(g["config_name"])
    cfg.data.dataset = g["dataset"]
    Cc = g["channels"]
    assert cfg.data.channels == Cc
    vm = VideoMetrics(cfg, preds_per_test=g["preds_per_test"])
    for ph in (1, 2):
        for bi, (pred, real) in enumerate(g["frames"][ph]):
            vm.update(pred.cuda(), real.cuda(), phase=ph)
            if ph in g["cannot"]:
                continue
            T = pred.shape[1] // Cc
            _, ssim, grey = frame_metrics(pred.cuda(), real[:, :Cc * T].cuda(), Cc, binary=vm.binary, return_grey=True)
            assert torch.equal(grey.cpu(), g["grey"][ph][bi])
            d = (ssim.cpu() - g["ssim"][ph][bi]).abs().max().item()
            print(f"  {case} phase {ph} batch {bi}: max |dSSIM| vs the real runner {d:.3e}")
            assert d <= SSIM_TOL
    got = vm.summary()
    if g["vid_metrics"] is None:
        assert got is None and vm.vid[1][0] == [0] * len(g["vid_mse_list"]) and g["vid_mse_list"] == [0] * len(g["vid_mse_list"])
        return
    for ph, key in ((1, ""), (2, "2")):
        if g["vid_mse" + key] is None:
            assert not vm.vid[ph][0]
            continue
        mine = np.array(vm.vid[ph][0], dtype=np.float64)
        gate = _mse_gates(g["vid_mse" + key], torch.cat(g["vid_mse64"][ph]).numpy())
        dm = np.abs(mine - g["vid_mse" + key].astype(np.float64))
        print(f"  {case} phase {ph}: per-video |dMSE| / gate max {(dm / gate).max():.3f}")
        assert np.all(dm <= gate)
        assert np.abs(np.array(vm.vid[ph][1]) - g["vid_ssim" + key]).max() <= SSIM_TOL
        ref = g["vid_mse" + key].astype(np.float64)
        _check_summary(got, g["vid_metrics"], gate.max(), ref.min(), float((LOG10E10 * np.log(1 / ref)).max()), sfx=key)
    want_keys = {k for k in g["vid_metrics"] if k != "ckpt" and "lpips" not in k}
    assert set(got) == want_keys and got["preds_per_test"] == g["preds_per_test"]


def test_through_video_gen_on_the_hip_path(golden_dir):
    """Task fixture B (tiny_spade, C = 3: (1) interpolation + (2) prediction with the future block masked) sampled on the HIP path as
    tests/test_gpu_video_tasks.py does, then VideoMetrics with phase 1 / 2 and preds_per_test 1 and 2 against tests/metrics_ref.py on the
    same HIP frames: per-frame SSIM 1e-9 and MSE 1 ulp (of the fp64 mean), per-video MSE within (T + 3) fp32 ulp of the restatement's
    (each frame within 1 ulp of the fp64 value on both sides, plus one rounding per fp32 add and the division), the summary within what
    that allows, and the reference's key names."""
    from mcvd_pytorch_amd import VideoMetrics, runner as r
    from mcvd_pytorch_amd.samplers import get_sampler
    from tests.test_gpu_video_tasks import _hip_net
    from tests.test_video_tasks_cpu import task_batch, task_calls, task_config, task_fixture, task_init
    g = task_fixture(golden_dir, "B")
    cfg = task_config(g)
    cfg.data.dataset = "Cityscapes"
    _, net = _hip_net(cfg)
    bound = get_sampler(cfg)
    X = task_batch(cfg, g)
    Cc = cfg.data.channels
    frames = {}
    for ph, (task, _) in enumerate(r.video_tasks(cfg), start=1):
        real, cond, cond_mask, nfp = r.task_conditioning(cfg, X, task)
        idx, seen = task_calls(g, task), []

        def sampler(x, scorenet, cond=None, **kw):
            call = idx[len(seen)]
            seen.append(call)
            return bound(x, scorenet, cond=cond, n_steps_each=0, step_lr=0.0, noise=g["step_noise"][call].cuda(), **kw)
        pred = r.video_gen(cfg, net, cond, sampler=sampler, task=task, cond_mask=cond_mask,
                           init_noise_fn=lambda i, shp, dev: task_init(g, idx, i, shp).to(dev))
        frames[ph] = (r.inverse_data_transform(cfg, pred), r.inverse_data_transform(cfg, real.cuda()))
    assert sorted(frames) == [1, 2]
    for ppt in (1, 2):
        vm = VideoMetrics(cfg, preds_per_test=ppt, scorenet=net)
        want = {"preds_per_test": ppt}
        for ph, sfx in ((1, ""), (2, "2")):
            pred, real = frames[ph]
            vm.update(pred, real, phase=ph)
            T = pred.shape[1] // Cc
            mse, ssim = _check_frames(pred.cpu(), real[:, :Cc * T].cpu(), Cc, False)
            ref_m, _, _, _ = metrics_ref.frame_metrics(pred.cpu(), real[:, :Cc * T].cpu(), Cc)
            rv_m, rv_s = metrics_ref.video_values(ref_m, ssim)
            rv_m = np.array([float(v) for v in rv_m], dtype=np.float32)
            mine = np.array(vm.vid[ph][0], dtype=np.float32)
            e = (T + 3) * _ulp32(rv_m)
            assert np.all(np.abs(mine.astype(np.float64) - rv_m) <= e)
            assert np.abs(np.array(vm.vid[ph][1]) - np.array(rv_s)).max() <= SSIM_TOL
            want.update(metrics_ref.summary(list(rv_m), rv_s, ppt, suffix=sfx))
            got = vm.summary()
            with np.errstate(divide="ignore"):
                psnr_max = float((10 * np.log10(1 / rv_m)).max())
            _check_summary(got, want, float(e.max()), float(rv_m.min()), psnr_max, sfx=sfx)
        assert set(vm.summary()) == set(want) == {"preds_per_test"} | {f"{m}{s}{t}" for m in ("mse", "psnr", "ssim") for s in ("", "2")
                                                                      for t in ("", "_std", "_conf95")}
