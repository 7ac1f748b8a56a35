"""GPU: the FVD path around the detector on the device -- mcvd_fvd_clips and mcvd_feature_stats (kernels/fvd.cpp) through
mcvd_pytorch_amd.metrics -- against tests/fvd_ref.py, numpy and what the REAL preprocess_single / frechet_distance /
NCSNRunner.video_gen computed (fixtures fvd_direct.pt, fvd_runner_{A,B,C}.pt; the CPU side is tests/test_fvd_cpu.py).

Gates:
  * fvd_clips against the fp64 restatement, every element: 8 x the fixture's ref_abs_dev -- the real preprocess_single's own fp32
    deviation from that restatement, measured when the fixture was made (2.2e-7); 8 is the factor LPIPS is held to here.  At S = 128 and
    S = 300 that is below what the product-rounded-first coordinate rule produces (3.4e-6, 1.3e-5; test_fvd_cpu.py checks it);
  * feature_stats against np.mean / np.cov in fp64, per element: 4 n 2^-53 (|Xc|^T |Xc|) / (n - 1) for sigma and 4 n 2^-53 sum|x| / n for
    the mean -- the standard bound between two differently ordered fp64 sums of n terms, derived, not measured;
  * frechet_distance and the summary keys: tests/test_fvd_cpu.py's relative 1e-10 (full rank) / 1e-7 (singular);
  * embeddings of the stand-in detector run under torch on the GPU: 8 x the fixture's feat_dev, the features' measured sensitivity to the
    resize's own fp32 rounding on the reference.
Measured ratios are printed by every test.
"""
import numpy as np
import pytest
import torch

from tests import fvd_ref
from tests.test_fvd_cpu import RTOL_SINGULAR, RUNNER_CASES, config_of, direct, features_of, rtol_of, runner

pytestmark = pytest.mark.gpu

GATE_FACTOR = 8
U = 2.0 ** -53


def _frames(seed, B, TC, S):
    return fvd_ref.make_frames(seed, B, TC, S)


def _clip_cases():
    """name -> (channels, parts on the host, row_step); parts that are channel slices of one tensor stay slices (read in place)."""
    cases = {}
    cases["c1_s64_cond2_pred3"] = (1, [_frames(1, 2, 2, 64), _frames(2, 2, 3, 64)], 1)
    cond = _frames(3, 4, 3 * 3, 128)                                   # cond_original: 2 cond frames + 1 future frame
    cases["c3_s128_cond2_pred2_future1_step2"] = (3, [cond[:, :6], _frames(4, 4, 6, 128), cond[:, -3:]], 2)
    cases["c3_s48"] = (3, [_frames(5, 1, 6, 48)], 1)
    cases["c3_s300_downscale"] = (3, [_frames(6, 1, 3, 300)], 1)
    cases["c1_s11"] = (1, [_frames(7, 3, 2, 11)], 2)
    return cases


@pytest.mark.parametrize("name", list(_clip_cases()))
def test_clips_against_the_fp64_restatement(golden_dir, name):
    from mcvd_pytorch_amd import fvd_clips
    g = direct(golden_dir)
    gate = GATE_FACTOR * g["ref_abs_dev"]
    Cc, parts, step = _clip_cases()[name]
    dev_parts = [p.cuda() for p in parts]
    if name.startswith("c3_s128"):                                   # slices of ONE device tensor, as cond_original's are: read in place
        cond = torch.cat([parts[0], parts[2]], 1).cuda()
        dev_parts = [cond[:, :6], parts[1].cuda(), cond[:, -3:]]
        assert not dev_parts[0].is_contiguous() and dev_parts[0].data_ptr() == cond.data_ptr()
    out = fvd_clips(dev_parts, Cc, row_step=step)
    again = fvd_clips(dev_parts, Cc, row_step=step)
    want = fvd_ref.clips64(parts, Cc, row_step=step)
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(want.shape) and out.shape[1:] == (3, sum(p.shape[1] for p in parts) // Cc, 224, 224)
    assert torch.equal(out, again), "two calls differ"
    dev = (out.double().cpu() - want).abs().max().item()
    print(f"  {name}: max |device - fp64| {dev:.3e} = {dev / g['ref_abs_dev']:.2f} x ref_abs_dev (gate {GATE_FACTOR})")
    assert dev <= gate
    if Cc == 1:
        assert torch.equal(out[:, 0], out[:, 1]) and torch.equal(out[:, 0], out[:, 2]), "grey planes differ"


def test_clip_parts_arrive_in_order():
    """Frame t of the output is source frame t of cond | pred | future, and row b is source row b * row_step."""
    from mcvd_pytorch_amd import fvd_clips
    B, S, Cc = 4, 16, 3
    frames = [2, 3, 1]
    parts, t0 = [], 0
    for n in frames:
        p = torch.empty(B, n * Cc, S, S)
        for b in range(B):
            for t in range(n):
                for c in range(Cc):
                    p[b, t * Cc + c] = (1 + c + 4 * (t0 + t) + 32 * b) / 256.0          # exact in fp32; a constant plane resizes to itself
        parts.append(p.cuda())
        t0 += n
    out = fvd_clips(parts, Cc, row_step=2).cpu()
    assert tuple(out.shape) == (2, 3, 6, 224, 224)
    for bi, b in enumerate((0, 2)):
        for t in range(6):
            for c in range(Cc):
                want = ((1 + c + 4 * t + 32 * b) / 256.0 - 0.5) * 2
                plane = out[bi, c, t]
                assert (plane - want).abs().max().item() <= 2.0 ** -22, (b, t, c)


def test_clips_hold_the_probes_of_the_real_preprocess_single(golden_dir):
    from mcvd_pytorch_amd import fvd_clips
    g = direct(golden_dir)
    gate = GATE_FACTOR * g["ref_abs_dev"]
    for c in g["resize"]:
        frames = fvd_ref.make_frames(c["frame_seed"], c["B"], c["T"] * c["channels"], c["S"])
        out = fvd_clips([frames.cuda()], c["channels"]).cpu()
        idx = fvd_ref.probe_index(out.numel(), g["probe_n"], c["probe_seed"])
        dev = (out.reshape(-1)[idx].double() - c["values"].double()).abs().max().item()
        dsum = abs(float(out.double().sum()) - c["sum"]) / out.numel()
        print(f"  S {c['S']} C {c['channels']}: probes {dev:.3e} = {dev / g['ref_abs_dev']:.2f} x ref_abs_dev, sum per element {dsum:.3e}")
        assert dev <= gate and dsum <= gate


def test_clips_refuse_what_the_reference_cannot_reshape():
    from mcvd_pytorch_amd import fvd_clips
    for parts, Cc in (([torch.zeros(1, 4, 16, 16)], 2),                # C = 2
                      ([torch.zeros(1, 3, 16, 20)], 3),                # not square
                      ([torch.zeros(1, 0, 16, 16)], 1),                # zero frames
                      ([torch.zeros(1, 2, 16, 16), torch.zeros(1, 0, 16, 16)], 1)):
        with pytest.raises(RuntimeError, match=r"code -1"):
            fvd_clips([p.cuda() for p in parts], Cc)
    with pytest.raises(ValueError):
        fvd_clips([], 1)


def _stats_case(rows, d, dtype, seed, wide=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, d + wide, generator=g, dtype=torch.float64) * (0.5 + torch.rand(d + wide, generator=g, dtype=torch.float64)) \
        + 0.3 * torch.randn(d + wide, generator=g, dtype=torch.float64)
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("rows,d,start,step,wide", [(2, 16, 0, 1, 0), (37, 33, 0, 1, 7), (1030, 400, 0, 1, 0), (96, 400, 1, 3, 0)])
def test_feature_stats_against_numpy(rows, d, start, step, wide, dtype):
    """(37, 33): d is no multiple of the 16-wide tiles and the matrix is a column slice (ld > d); 1030 rows: several row chunks."""
    from mcvd_pytorch_amd import feature_stats
    x = _stats_case(rows, d, dtype, 100 + rows, wide)
    xd = x.cuda()[:, :d]
    mu, sigma = feature_stats(xd, start, step)
    mu2, sigma2 = feature_stats(xd, start, step)
    assert mu.dtype == torch.float64 and sigma.dtype == torch.float64 and tuple(mu.shape) == (d,) and tuple(sigma.shape) == (d, d)
    assert torch.equal(mu, mu2) and torch.equal(sigma, sigma2), "two calls differ"
    assert torch.equal(sigma, sigma.t()), "sigma is not exactly symmetric"
    sel = x[start::step, :d].double().numpy()
    n = len(sel)
    want_mu, want_sigma = fvd_ref.stats_np(sel)
    xc = np.abs(sel - want_mu)
    bound_sigma = 4 * n * U * (xc.T @ xc) / (n - 1)
    bound_mu = 4 * n * U * np.abs(sel).sum(0) / n
    r_mu = (np.abs(mu.cpu().numpy() - want_mu) / bound_mu).max()
    r_sigma = (np.abs(sigma.cpu().numpy() - want_sigma) / bound_sigma).max()
    print(f"  ({rows}, {d}) [{start}::{step}] {dtype}: mean {r_mu:.3f}, sigma {r_sigma:.3f} of the bound")
    assert r_mu <= 1.0 and r_sigma <= 1.0


def test_feature_stats_refuses_one_row_and_wide_features():
    from mcvd_pytorch_amd import feature_stats
    x = torch.randn(6, 16).cuda()
    for args in ((x[:1], 0, 1), (x, 5, 1), (x, 0, 6), (torch.randn(4, 2049).cuda(), 0, 1)):
        with pytest.raises(RuntimeError, match=r"code -1"):
            feature_stats(*args)


def test_frechet_distance_on_the_device(golden_dir):
    from mcvd_pytorch_amd import frechet_distance
    for spec in direct(golden_dir)["features"]:
        fake, real = features_of(spec)
        got = frechet_distance(fake.cuda(), real.cuda(), spec["start"], spec["step"])
        rel = abs(got - spec["value"]) / spec["value"]
        print(f"  {spec['name']}: {got!r} against {spec['value']!r}: relative {rel:.3e} = {rel / rtol_of(spec['full_rank']):.3f} of the gate")
        assert rel <= rtol_of(spec["full_rank"]), spec["name"]


def _feed(vm, g):
    """The runner's call order per batch: (1), then (2) where it ran, then (3)."""
    for i in range(g["iters"]):
        vm.update(g["pred_1"][i].cuda(), g["real_1"][i].cuda(), phase=1, cond01=g["cond_1"][i].cuda())
        if g["second_calc"]:
            vm.update(g["pred_2"][i].cuda(), g["real_2"][i].cuda(), phase=2, cond01=g["cond_2"][i].cuda())
        if g["gates"][2]:
            vm.update_gen(g["pred_3"][i].cuda())


@pytest.mark.parametrize("case", RUNNER_CASES)
def test_embeddings_with_the_stand_in_detector_on_the_gpu(golden_dir, case):
    """Clips built on the device, the stand-in run under torch on the GPU: the runner's embeddings, in its order and count."""
    from mcvd_pytorch_amd import VideoMetrics
    g = runner(golden_dir, case)
    det = fvd_ref.StandInDetector(g["seed"]).cuda().eval()
    seen = []

    def detector(x, **kw):
        assert kw == dict(rescale=False, resize=False, return_features=True)
        assert x.is_cuda and x.dtype == torch.float32 and x.shape[1] == 3 and x.shape[3:] == (224, 224) and len(x) <= 10
        seen.append(tuple(x.shape))
        return det(x, **kw)
    vm = VideoMetrics(config_of(g), preds_per_test=g["preds_per_test"], fvd=detector)
    _feed(vm, g)
    # the fixture's calls hold the [rows, 3, T, S, S] clips get_fvd_feats was handed, before preprocess_single
    assert seen == [tuple(shape[:3]) + (224, 224) for shape, _ in g["calls"]], "the detector saw other clips than the reference's"
    e = vm.embeddings()
    gate = GATE_FACTOR * g["feat_dev"]
    for k, ref in g["embeddings"].items():
        if len(ref) == 0:
            assert len(e[k]) == 0, k
            continue
        assert e[k].dtype == np.float64 and e[k].shape == tuple(ref.shape), (k, e[k].shape, tuple(ref.shape))
        dev = np.abs(e[k] - ref.numpy()).max()
        print(f"  {case} {k} {e[k].shape}: {dev:.3e} = {dev / g['feat_dev']:.2f} x feat_dev (gate {GATE_FACTOR})")
        assert dev <= gate, k
    ppt = g["preds_per_test"]
    assert len(e["real_embeddings"]) * ppt == len(e["fake_embeddings"]), "real rows are repeated"
    if g["gates"][2]:
        reused = e["real_embeddings2"] if g["second_calc"] else e["real_embeddings"]
        assert np.array_equal(e["real_embeddings3"], reused), "phase (3) does not reuse the batch's real embeddings"
    assert vm.summary() is not None


def test_detector_batches(golden_dir):
    """fvd_batch clips per detector call, the rest in a last smaller one (get_feats, fvd.py:47-48)."""
    from mcvd_pytorch_amd import VideoMetrics
    g = runner(golden_dir, "C")
    det = fvd_ref.StandInDetector(g["seed"]).cuda().eval()
    seen = []

    def detector(x, **kw):
        seen.append(len(x))
        return det(x, **kw)
    vm = VideoMetrics(config_of(g), preds_per_test=g["preds_per_test"], fvd=detector, fvd_batch=3)
    _feed(vm, g)
    assert seen == [2, 3, 1, 3, 1] * g["iters"]
    ref = g["embeddings"]["fake_embeddings3"].numpy()
    assert np.abs(vm.embeddings()["fake_embeddings3"] - ref).max() <= GATE_FACTOR * g["feat_dev"]


@pytest.mark.parametrize("case", RUNNER_CASES)
def test_summary_from_the_replayed_embeddings(golden_dir, case):
    """The reference's features handed back by a detector stub, call by call: clips, statistics and distances on the device, and the
    runner's fvd / fvd2 / fvd3 groups within the Frechet gates (no tolerance that is not the reference's lands on the end value)."""
    from mcvd_pytorch_amd import VideoMetrics
    g = runner(golden_dir, case)
    n_call = [0]

    def stub(x, **kw):
        feats = g["call_feats"][n_call[0]]
        n_call[0] += 1
        assert len(feats) == len(x)
        return feats.cuda()
    vm = VideoMetrics(config_of(g), preds_per_test=g["preds_per_test"], fvd=stub)
    _feed(vm, g)
    assert n_call[0] == len(g["call_feats"])
    out = vm.summary()
    assert [k for k in out if k.startswith("fvd")] == g["fvd_keys"]
    assert list(out) == [k for k in g["vid_metrics"] if k != "ckpt" and not k.startswith("lpips")]
    for k in g["fvd_keys"]:
        want, got = g["vid_metrics"][k], out[k]
        if g["preds_per_test"] == 1 and "traj" in k:
            assert want == -1 and got == -1
            continue
        scale = abs(g["vid_metrics"][k.split("_")[0]]) if ("std" in k or "conf95" in k) else abs(want)
        print(f"  {case} {k}: {got!r} against {want!r}: {abs(got - want) / scale:.3e} (gate {RTOL_SINGULAR})")
        assert abs(got - want) <= RTOL_SINGULAR * scale, k
