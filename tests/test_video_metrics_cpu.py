"""CPU: video_gen's test-mode metrics (MSE, PSNR, SSIM).  tests/metrics_ref.py (the torch float64 restatement) against scipy / Pillow
where they are installed and against what the REAL `NCSNRunner.video_gen` computed (tools/gen_video_metrics_golden.py ran its metric
loop and summary, runners/ncsn_runner.py:1580-1609, :1749-1778, :2195-2255); mcvd_pytorch_amd.metrics' host aggregation against the
recorded summary.

    smmnist     SMMNIST-named (MNIST rule), C = 1, preds_per_test 2, two batches    (1) prediction
    cityscapes  C = 3 (quantisation + Pillow's luma)                               (1) interpolation + (2) prediction, future masked
    beyond      clips shorter than the prediction                                  (1) "cannot calculate": zeros, no summary
"""
import math

import numpy as np
import pytest
import torch

from tests import metrics_ref
from tests.golden_io import load_golden

CASES = ["smmnist", "cityscapes", "beyond"]


def fixture(golden_dir, case):
    return load_golden(golden_dir, f"video_metrics_{case}.pt")


def _binary(g):
    return g["dataset"].upper() in metrics_ref.MNIST


def _ulp32(x):
    x = np.abs(np.asarray(x, dtype=np.float32))
    return np.spacing(x).astype(np.float64)


def test_restated_moments_match_scipy_gaussian_filter():
    """The restatement's Gaussian moments equal scipy.ndimage.gaussian_filter(sigma=1.5, truncate=3.5) -- the call skimage makes -- on
    the cropped interior, within 1e-12 relative (fp64; the two sum the 11 taps in different orders)."""
    ndimage = pytest.importorskip("scipy.ndimage")
    g = torch.Generator().manual_seed(5)
    for H, W in ((11, 12), (32, 32), (37, 64)):
        a = torch.randint(0, 256, (H, W), generator=g).double()
        for v in (a, a * a, a * torch.roll(a, 1, 0)):
            ours = metrics_ref.moments(v[None])[0].numpy()
            want = ndimage.gaussian_filter(v.numpy(), sigma=1.5, truncate=3.5)[5:-5, 5:-5]
            assert ours.shape == want.shape
            assert np.max(np.abs(ours - want) / np.maximum(np.abs(want), 1e-300)) <= 1e-12


def test_luma_formula_matches_pillow_on_every_rgb_triple():
    """Pillow's RGB -> L on all 2^24 triples equals (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    Image = pytest.importorskip("PIL.Image")
    k = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
    want = np.asarray(Image.fromarray(rgb, mode="RGB").convert("L"))
    t = torch.from_numpy(rgb.astype(np.int64))
    got = metrics_ref.luma(t[..., 0], t[..., 1], t[..., 2]).numpy().astype(np.uint8)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_real_runner(golden_dir, case):
    """Given the frames the real runner's metric loop saw: the grey planes equal the real-Pillow planes exactly, the per-frame SSIM is
    within 1e-12 of the scipy-based restatement's value inside the real runner, and the per-frame MSE within 1 fp32 ulp of F.mse_loss."""
    g = fixture(golden_dir, case)
    C = g["channels"]
    n = 0
    for ph in (1, 2):
        if ph in g["cannot"]:
            continue
        for k, (pred, real) in enumerate(g["frames"][ph]):
            T = pred.shape[1] // C
            mse, ssim, gp, gr = metrics_ref.frame_metrics(pred, real[:, :C * T], C, binary=_binary(g))
            assert torch.equal(gp, g["grey"][ph][k][0]) and torch.equal(gr, g["grey"][ph][k][1])
            assert (ssim - g["ssim"][ph][k]).abs().max().item() <= 1e-12
            assert np.all(np.abs(mse.numpy().astype(np.float64) - g["mse"][ph][k].numpy()) <= _ulp32(g["mse"][ph][k].numpy()))
            n += 1
    assert n == (0 if case == "beyond" else {"smmnist": 2, "cityscapes": 2}[case])


@pytest.mark.parametrize("case", CASES)
def test_host_aggregation_reproduces_the_summary(golden_dir, case):
    """mcvd_pytorch_amd.metrics' per-video values and summary, fed the per-frame values the real runner computed: the vid lists and
    the mse / psnr / ssim arrays handed to image_metric_stuff are bit-identical (same ops, same dtypes, same order); mean and std are
    bit-identical; conf95 equals scipy's (the normal quantile is scipy's own ndtri((1 - 0.95) / 2), as a constant)."""
    from mcvd_pytorch_amd import metrics
    g = fixture(golden_dir, case)
    ppt = g["preds_per_test"]
    lists = {}
    for ph in (1, 2):
        vm, vs = [], []
        for bi, (pred, real) in enumerate(g["frames"][ph]):
            if ph in g["cannot"]:
                vm += [0] * len(pred)
                vs += [0] * len(pred)
            else:
                m, s = metrics.video_values(g["mse"][ph][bi], g["ssim"][ph][bi])
                vm += m
                vs += s
        lists[ph] = (vm, vs)
    assert np.array(lists[1][0]).dtype == g["vid_mse"].dtype
    assert np.array_equal(np.array(lists[1][0]), g["vid_mse"]) and np.array_equal(np.array(lists[1][1]), g["vid_ssim"])
    if g["vid_mse2"] is not None:
        assert np.array_equal(np.array(lists[2][0]), g["vid_mse2"]) and np.array_equal(np.array(lists[2][1]), g["vid_ssim2"])
    if g["vid_metrics"] is None:                                  # the runner returned None: (1) could not calculate
        assert case == "beyond" and 1 in g["cannot"] and all(v == 0 for v in lists[1][0])
        return
    want = g["vid_metrics"]
    got = metrics.summarize(*lists[1], ppt)
    arrays = [a for a in g["metric_arrays"]]
    if g["vid_mse2"] is not None:
        got.update(metrics.summarize(*lists[2], ppt, suffix="2"))
    # image_metric_stuff's calls in order: mse, psnr, ssim, lpips (then the same with 2)
    order = ["mse", "psnr", "ssim", None] + (["mse2", "psnr2", "ssim2", None] if g["vid_mse2"] is not None else [])
    assert len(arrays) == len(order)
    recomputed = {}
    for ph, sfx in ((1, ""), (2, "2")):
        if ph == 2 and g["vid_mse2"] is None:
            continue
        vm = np.array(lists[ph][0])
        recomputed["mse" + sfx] = vm.reshape(-1, ppt).min(-1)
        with np.errstate(divide="ignore"):
            recomputed["psnr" + sfx] = (10 * np.log10(1 / vm)).reshape(-1, ppt).max(-1)
        recomputed["ssim" + sfx] = np.array(lists[ph][1]).reshape(-1, ppt).max(-1)
    for name, arr in zip(order, arrays):
        if name is not None:
            assert arr.dtype == recomputed[name].dtype and np.array_equal(arr, recomputed[name]), name
    for k, v in got.items():
        if k.endswith("_conf95"):
            assert (math.isnan(v) and math.isnan(want[k])) or v == want[k], (k, v, want[k])
        else:
            assert v == want[k] or (math.isnan(v) and math.isnan(want[k])), (k, v, want[k])
    assert set(got) == {k for k in want if k not in ("ckpt",) and "lpips" not in k} - {"preds_per_test"}


def test_conf95_constant_is_scipys_quantile():
    special = pytest.importorskip("scipy.special")
    from mcvd_pytorch_amd import metrics
    assert metrics._NDTRI_Q1 == float(special.ndtri((1.0 - 0.95) / 2))


def test_conf95_matches_scipy_interval_on_edge_cases():
    """scipy's ppf rules: nan where the scale (sem) is 0 or nan, or the location is nan; otherwise avg - (ndtri(q) * sem + avg)."""
    stats = pytest.importorskip("scipy.stats")
    from mcvd_pytorch_amd import metrics
    g = np.random.default_rng(3)
    for arr in (g.random(7).astype(np.float32), g.random(5), np.zeros(4, dtype=np.int64), np.full(3, np.inf, dtype=np.float32),
                np.array([0.5], dtype=np.float32), np.array([1.0, 2.0, np.nan])):
        with np.errstate(all="ignore"):
            avg = arr.mean().item()
            want = avg - float(stats.norm.interval(0.95, loc=avg, scale=stats.sem(arr))[0])
            got = metrics.image_metric_stuff(arr)[2]
        assert (math.isnan(got) and math.isnan(want)) or got == want, (arr, got, want)


def test_restated_summary_matches_the_real_runner(golden_dir):
    """tests/metrics_ref.summary (the standard library's normal quantile instead of scipy's) against the recorded summaries: the lists
    and mean / std exactly; conf95 = avg - (z * sem + avg) within 4 ulp of max(|avg|, |conf95|): statistics.NormalDist's quantile z may
    differ from ndtri's in the last bit, which moves z * sem (|z * sem| = |conf95|) by an ulp, and the sum and the difference after it
    round once each."""
    for case in ("smmnist", "cityscapes"):
        g = fixture(golden_dir, case)
        got = metrics_ref.summary(list(g["vid_mse"]), list(g["vid_ssim"]), g["preds_per_test"])
        if g["vid_mse2"] is not None:
            got.update(metrics_ref.summary(list(g["vid_mse2"]), list(g["vid_ssim2"]), g["preds_per_test"], suffix="2"))
        for k, v in got.items():
            w = g["vid_metrics"][k]
            tol = 4 * np.spacing(max(abs(g["vid_metrics"][k[:-len("_conf95")]]), abs(w))) if k.endswith("_conf95") else 0.0
            assert abs(v - w) <= tol, (case, k, v, w)


def test_frame_metrics_refuses_unsupported_frames_without_touching_the_device():
    """C = 2 / 4 (torchvision's LA / RGBA) and frames below the 11 x 11 window raise ValueError before any device work."""
    from mcvd_pytorch_amd import frame_metrics
    with pytest.raises(ValueError):
        frame_metrics(torch.zeros(1, 2, 16, 16), torch.zeros(1, 2, 16, 16), 2)
    with pytest.raises(ValueError):
        frame_metrics(torch.zeros(1, 4, 16, 16), torch.zeros(1, 4, 16, 16), 4)
    with pytest.raises(ValueError):
        metrics_ref.ssim_planes(torch.zeros(1, 10, 16, dtype=torch.uint8), torch.zeros(1, 10, 16, dtype=torch.uint8))
