"""CPU: LPIPS of video_gen's test mode.  tests/lpips_ref.py (integer resize + torch float64 restatement) against Pillow where it is
installed and against what the REAL `eval_models.PerceptualLoss` / `NCSNRunner.video_gen` computed over a seeded AlexNet backbone
(fixtures tests/golden/lpips_direct.pt, lpips_runner_{smmnist,cityscapes}.pt; tools/gen_lpips_golden.py); mcvd_pytorch_amd.metrics' host
aggregation against the recorded lists and summary.

Each fixture carries ref_rel_dev: the largest |fp32 - fp64| / fp64 over its frame values, the real net's fp32 result against the fp64
restatement, measured when the fixture was made (2.0e-7 ... a few e-7).  The restatement, run again here, must land within it (times 1 + 1e-3: the fp64 sums themselves move by ~1e-13 with the thread count).
"""
import math

import numpy as np
import pytest
import torch

from tests import lpips_ref
from tests.golden_io import load_golden

RUNNER_CASES = ["smmnist", "cityscapes"]


def direct(golden_dir):
    return load_golden(golden_dir, "lpips_direct.pt")


def runner(golden_dir, case):
    return load_golden(golden_dir, f"lpips_runner_{case}.pt")


@pytest.mark.parametrize("in_size", [16, 32, 48, 64, 96, 128, 200, 256])
def test_integer_resize_equals_pillow(in_size):
    """The restated two-pass 8-bit fixed-point resize equals PIL's Image.resize((128, 128), BILINEAR) bit for bit on random uint8 planes,
    for in_size -> 128 along the width, along the height, and along both (L and RGB images)."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(in_size)
    for H, W in ((in_size, in_size), (in_size, 128), (128, in_size), (in_size, 77)):
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        want = np.asarray(Image.fromarray(a, mode="RGB").resize((128, 128), Image.BILINEAR))
        got = lpips_ref.resize_u8(np.moveaxis(a, -1, 0))
        assert np.array_equal(np.moveaxis(got, 0, -1), want), (H, W)
        wl = np.asarray(Image.fromarray(a[:, :, 0], mode="L").resize((128, 128), Image.BILINEAR))
        assert np.array_equal(lpips_ref.resize_u8(a[:, :, 0]), wl), (H, W)
    edge = np.zeros((in_size, in_size), np.uint8)
    edge[:, in_size // 2:] = 255
    assert np.array_equal(lpips_ref.resize_u8(edge), np.asarray(Image.fromarray(edge, mode="L").resize((128, 128), Image.BILINEAR)))


def test_integer_resize_equals_the_stored_pillow_planes(golden_dir):
    """No Pillow needed: every resized plane the fixture recorded from the real Pillow (32, 64, 128, 256 -> 128; C = 1 and 3)."""
    g = direct(golden_dir)
    sizes = set()
    for c in g["cases"]:
        fr = g[f"frames_{c['name']}"]
        got = torch.stack([lpips_ref.resized_planes(fr[0], c["channels"]), lpips_ref.resized_planes(fr[1], c["channels"])])
        assert torch.equal(got, g[f"resized_{c['name']}"]), c["name"]
        sizes.add(fr.shape[-1])
    assert sizes == {32, 64, 128, 256}


def test_regenerated_backbone_matches_the_stored_probes(golden_dir):
    """A drift of torch's generator shows up here as 'weights differ', not as a kernel failure."""
    for g in [direct(golden_dir)] + [runner(golden_dir, c) for c in RUNNER_CASES]:
        assert g["recipe"] == lpips_ref.RECIPE
        probes = lpips_ref.backbone_probe(lpips_ref.make_backbone(g["seed"]))
        assert set(probes) == set(g["probes"])
        for k, (s, v) in probes.items():
            # the probed values exactly; the fp64 sum to 1e-8 absolute (its order of addition depends on the thread count: the tensors hold
            # up to 9e5 values of magnitude < 1, so orders differ by ~1e-11; one changed weight moves the sum by ~1e-2)
            assert torch.equal(v, g["probes"][k][1]) and abs(s - g["probes"][k][0]) <= 1e-8, f"weights differ: {k}"


def test_state_dict_names_are_the_real_pnetlin_names(golden_dir):
    """The parameter names the C ABI accepts are those of the real PNetLin.state_dict(), recorded when the fixture was made."""
    names = direct(golden_dir)["state_dict_names"]
    want = ["scaling_layer.shift", "scaling_layer.scale"]
    for idx, sl, *_ in lpips_ref.CONVS:
        want += [f"net.{sl}.weight", f"net.{sl}.bias"]
    want += [f"lin{k}.model.1.weight" for k in range(5)]
    assert sorted(names) == sorted(want)


def test_restatement_lands_within_ref_rel_dev_of_the_real_net(golden_dir):
    """lpips_ref in fp64 on the regenerated backbone against every fp32 frame and per-tap value of the real PNetLin: within ref_rel_dev
    (frame values; per-tap values within the sanity cap 1e-4 the generator applies); the identical pair is exactly 0 on both sides; the two
    stored tap sets agree to 1e-5 of their norm."""
    g = direct(golden_dir)
    bb = lpips_ref.make_backbone(g["seed"])
    assert 0 < g["ref_rel_dev"] <= 1e-4
    n_zero = 0
    for c in g["cases"]:
        name, fr = c["name"], g[f"frames_{c['name']}"]
        v64, pt64, _ = lpips_ref.frame_lpips64(fr[0], fr[1], c["channels"], bb, g["lins"], g["shift"], g["scale"])
        assert torch.equal(v64, g[f"value64_{name}"]) or (v64 - g[f"value64_{name}"]).abs().max() <= 1e-13 * v64.abs().max()
        v32 = g[f"value_{name}"].double()
        zero = v64 == 0
        n_zero += int(zero.sum())
        assert torch.equal(v32[zero], v64[zero])
        dev = ((v32[~zero] - v64[~zero]).abs() / v64[~zero]).max().item()
        print(f"  {name}: real fp32 vs fp64 restatement {dev:.3e} (ref_rel_dev {g['ref_rel_dev']:.3e})")
        assert dev <= g["ref_rel_dev"] * (1 + 1e-3)
        p32 = g[f"per_tap_{name}"].double()
        nz = pt64 != 0
        assert ((p32[nz] - pt64[nz]).abs() / pt64[nz]).max().item() <= 1e-4 and torch.equal(p32[~nz], pt64[~nz])
    assert n_zero == 1
    cases = {c["name"]: c for c in g["cases"]}
    for ti, (cn, which, b, t) in enumerate(g["tap_images"]):
        Cc = cases[cn]["channels"]
        x = lpips_ref.net_input(g[f"resized_{cn}"][which, b, t][None])
        for k, tp in enumerate(lpips_ref.taps(x, bb, g["shift"], g["scale"])):
            ref = g[f"tap{k + 1}_real"][ti].double()
            assert tp[0].shape == ref.shape and Cc in (1, 3)
            assert (tp[0] - ref).norm() <= 1e-5 * ref.norm()


@pytest.mark.parametrize("case", RUNNER_CASES)
def test_restatement_lands_within_ref_rel_dev_of_the_real_runner(golden_dir, case):
    from tests.test_video_metrics_cpu import fixture
    g, frames = runner(golden_dir, case), fixture(golden_dir, case)["frames"]
    bb = lpips_ref.make_backbone(g["seed"])
    Cc = g["channels"]
    n = 0
    for ph in (1, 2):
        assert len(g["value"][ph]) == len(frames[ph])
        for bi, (pred, real) in enumerate(frames[ph]):
            v64, _, _ = lpips_ref.frame_lpips64(pred, real[:, :pred.shape[1]], Cc, bb, g["lins"], g["shift"], g["scale"])
            dev = ((g["value"][ph][bi].double() - v64).abs() / v64).max().item()
            assert dev <= g["ref_rel_dev"] * (1 + 1e-3) <= 1e-4
            n += 1
    assert n == 2


@pytest.mark.parametrize("case", RUNNER_CASES)
def test_host_aggregation_reproduces_the_runner(golden_dir, case):
    """metrics.video_lpips and summarize_lpips, fed the fp32 frame values the real runner computed, give vid_lpips, the arrays handed to
    image_metric_stuff and the lpips keys of vid_metrics to the last bit (the same operations in the same dtypes and order)."""
    from mcvd_pytorch_amd import metrics
    g = runner(golden_dir, case)
    ppt = g["preds_per_test"]
    arrays = g["metric_arrays"]
    assert len(arrays) == (8 if g["vid_lpips2"] else 4)
    for ph, sfx, key, ai in ((1, "", "vid_lpips", 3), (2, "2", "vid_lpips2", 7)):
        if not g["value"][ph]:
            assert g[key] is None
            continue
        vid = [v for vals in g["value"][ph] for v in metrics.video_lpips(vals)]
        assert vid == g[key] and all(isinstance(v, float) for v in vid)
        assert vid == [v for vals in g["value"][ph] for v in lpips_ref.video_lpips(vals)]
        arr = np.array(vid).reshape(-1, ppt).min(-1)
        assert arr.dtype == arrays[ai].dtype and np.array_equal(arr, arrays[ai])
        got = metrics.summarize_lpips(vid, ppt, suffix=sfx)
        assert set(got) == {f"lpips{sfx}", f"lpips{sfx}_std", f"lpips{sfx}_conf95"}
        for k, v in got.items():
            w = g["vid_metrics"][k]
            assert v == w or (math.isnan(v) and math.isnan(w)), (k, v, w)
    if case == "smmnist":
        assert ppt == 2


def test_video_metrics_without_lpips_keeps_its_key_set():
    """VideoMetrics without lpips= returns exactly the old keys; with an LpipsNet the six lpips keys join them (host logic only)."""
    from mcvd_pytorch_amd import metrics
    from oracle import synth
    vm = metrics.VideoMetrics(synth.make_config("tiny"), preds_per_test=1)
    assert vm.lpips is None
    vm.vid[1][0].extend([np.float32(0.1), np.float32(0.2)])
    vm.vid[1][1].extend([0.5, 0.6])
    vm.vid[2][0].extend([np.float32(0.1), np.float32(0.3)])
    vm.vid[2][1].extend([0.5, 0.7])
    old = {"preds_per_test"} | {f"{m}{s}{t}" for m in ("mse", "psnr", "ssim") for s in ("", "2") for t in ("", "_std", "_conf95")}
    assert set(vm.summary()) == old
    vm.lpips = object()
    vm.vid_lpips[1].extend([0.3, 0.4])
    vm.vid_lpips[2].extend([0.3, 0.5])
    s = vm.summary()
    assert set(s) == old | {f"lpips{x}{t}" for x in ("", "2") for t in ("", "_std", "_conf95")}
    assert s["lpips"] == np.array([0.3, 0.4]).mean().item()


def test_frame_lpips_refuses_unsupported_channels_without_touching_the_device():
    from mcvd_pytorch_amd import frame_lpips
    with pytest.raises(ValueError):
        frame_lpips(torch.zeros(1, 2, 16, 16), torch.zeros(1, 2, 16, 16), 2, None)
