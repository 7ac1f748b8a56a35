"""GPU: the FID InceptionV3 on the device -- mcvd_inception_* and mcvd_op_resize299 (kernels/inception.cpp), mcvd_op_conv2d_rect,
mcvd_op_pool3 and mcvd_op_global_avg (the detector nets' shared ops, kernels/detector_ops.cpp) and metrics.FidInception -- against fp64 torch, against tests/inception_ref.py (the fp64 restatement) and against
what the REAL evaluation.inception.InceptionV3 computed over the seeded weights (fixture fid_inception.pt; tests/test_fid_inception_cpu.py).

Gates (none is a figure of the code under test):
  * mcvd_op_conv2d_rect against F.conv2d in fp64: per output |y - y64| <= (K + 4) 2^-24 (|alpha| sum |w| |x| + |beta|) -- the bound of a
    K-term fp32 fma chain plus the epilogue's fma and the rounding of the result;
  * average pool: 2^-22 x (sum |x| over the window) / count; max pool: exact; global average: within 1 ulp of the fp64 mean;
  * resize: against torch's own fp32 values stored in the fixture, max |y - torch| / max |torch| <= 8 x the stored deviation of torch's
    fp32 result from its fp64 result (the FVD row's rule); 299 -> 299 is bit-identical to 2 x - 1;
  * the whole net: per block max |y - y64| / max |y64| <= GATE_FACTOR = 8 x the fixture's ref_rel_dev of that block, the real module's
    own fp32 result measured against the fp64 restatement when the fixture was made -- this project's standing margin over the
    reference's own fp32 error.  Both are fp32 roundings of the same sums in different orders.
  * batch, chunk, slice and repeat invariance: bit-identical.
Measured ratios are printed by every test.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import inception_ref as ir
from tests.hiputil import Ctx, P
from tests.test_fid_inception_cpu import fixture, images, restated, weights

pytestmark = pytest.mark.gpu

GATE_FACTOR = 8
ESTATE = -3
SENTINEL = -12345.0


@functools.lru_cache(maxsize=None)
def _ctx():
    return Ctx()


@functools.lru_cache(maxsize=None)
def detector(seed, blocks):
    """One FidInception per block set for the whole module: loading 87 MB of weights is not what the tests are about."""
    from mcvd_pytorch_amd import FidInception
    return FidInception(output_blocks=blocks, device="cuda:0").load_state_dict(weights(seed))


def conv_rect(x, w, alpha, beta, stride, ph, pw, relu, out=None, c0=0):
    from mcvd_pytorch_amd import _lib
    B, Cin, H, W = x.shape
    Cout, _, kh, kw = w.shape
    OH, OW = (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1
    y = torch.full((B, Cout, OH, OW), float("nan"), device="cuda") if out is None else out
    _lib.check(_lib.lib.mcvd_op_conv2d_rect(_ctx().h, P(x), P(w), P(alpha), P(beta), B, Cin, H, W, Cout, kh, kw, stride, ph, pw, relu, P(y), c0,
                                            y.shape[1]), "op_conv2d_rect")
    return y


# (id, kh, kw, stride, ph, pw, H, W, Cin, Cout, N, relu): each breaks one tiling assumption
CONV_CASES = [
    ("k1x7", 1, 7, 1, 0, 3, 17, 17, 20, 70, 3, 1),          # K = 140, Cout 70, 867 pixels: no tile multiple anywhere
    ("k7x1", 7, 1, 1, 3, 0, 17, 17, 20, 70, 3, 1),
    ("k1x3", 1, 3, 1, 0, 1, 8, 8, 24, 40, 5, 1),            # rectangular taps on a small map
    ("k3x1", 3, 1, 1, 1, 0, 8, 8, 24, 40, 5, 0),
    ("k3s2_35", 3, 3, 2, 0, 0, 35, 35, 16, 48, 2, 1),       # stride 2 on odd maps: 35 -> 17
    ("k3s2_17", 3, 3, 2, 0, 0, 17, 17, 16, 48, 2, 0),       # 17 -> 8
    ("k3s2_31", 3, 3, 2, 0, 0, 31, 31, 3, 32, 2, 1),        # K = 27, the 32-channel tile with a gather
    ("k5p2", 5, 5, 1, 2, 2, 35, 35, 12, 64, 1, 1),          # large square taps
    ("k1_deep", 1, 1, 1, 0, 0, 8, 8, 2048, 64, 1, 1),       # deep K, 64 pixels: less than one tile
    ("k1_c32", 1, 1, 1, 0, 0, 35, 35, 48, 32, 2, 1),        # the 32-channel tile on the 1 x 1 path
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv2d_rect_against_fp64(case):
    name, kh, kw, stride, ph, pw, H, W, Cin, Cout, N, relu = case
    gen = torch.Generator().manual_seed(1000 * Cin + 10 * kh + kw)
    x = torch.randn(N, Cin, H, W, generator=gen)
    K = Cin * kh * kw
    w = torch.randn(Cout, Cin, kh, kw, generator=gen) / K ** 0.5
    alpha = (0.5 + torch.rand(Cout, generator=gen)) * torch.where(torch.rand(Cout, generator=gen) < 0.25, -1.0, 1.0)
    beta = 0.3 * torch.randn(Cout, generator=gen)
    a64, b64 = alpha.double().reshape(1, -1, 1, 1), beta.double().reshape(1, -1, 1, 1)
    want = a64 * F.conv2d(x.double(), w.double(), None, stride=stride, padding=(ph, pw)) + b64
    if relu:
        want = want.relu()
    mag = a64.abs() * F.conv2d(x.double().abs(), w.double().abs(), None, stride=stride, padding=(ph, pw)) + b64.abs()
    xc, wc, ac, bc = x.cuda(), w.cuda(), alpha.cuda(), beta.cuda()
    y = conv_rect(xc, wc, ac, bc, stride, ph, pw, relu)
    ratio = ((y.cpu().double() - want).abs() / mag).max().item() / ((K + 4) * 2.0 ** -24)
    print(f"  conv_rect {name}: worst error / bound {ratio:.3f}")
    assert torch.isfinite(y).all() and ratio <= 1.0
    # the same call again, and image 0 alone: the same bits
    assert torch.equal(conv_rect(xc, wc, ac, bc, stride, ph, pw, relu), y)
    assert torch.equal(conv_rect(xc[:1].contiguous(), wc, ac, bc, stride, ph, pw, relu)[0], y[0])
    # without alpha and beta the epilogue is the identity on the chain's value
    if name == "k1x3":
        plain = conv_rect(xc, wc, None, None, stride, ph, pw, 0)
        p64 = F.conv2d(x.double(), w.double(), None, stride=stride, padding=(ph, pw))
        pm = F.conv2d(x.double().abs(), w.double().abs(), None, stride=stride, padding=(ph, pw))
        assert ((plain.cpu().double() - p64).abs() / pm).max().item() <= (K + 4) * 2.0 ** -24


def test_conv2d_rect_stores_its_channel_slice_only():
    """Cout 40 into channels [24, 64) of a 96-channel tensor pre-filled with a sentinel: the slice holds the stand-alone result's bits and
    every sentinel outside it is intact."""
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(5, 24, 8, 8, generator=gen).cuda()
    w = (torch.randn(40, 24, 1, 3, generator=gen) / 72 ** 0.5).cuda()
    alpha, beta = (0.5 + torch.rand(40, generator=gen)).cuda(), (0.1 * torch.randn(40, generator=gen)).cuda()
    alone = conv_rect(x, w, alpha, beta, 1, 0, 1, 1)
    wide = torch.full((5, 96, 8, 8), SENTINEL, device="cuda")
    conv_rect(x, w, alpha, beta, 1, 0, 1, 1, out=wide, c0=24)
    assert torch.equal(wide[:, 24:64], alone)
    assert (wide[:, :24] == SENTINEL).all() and (wide[:, 64:] == SENTINEL).all()


@pytest.mark.parametrize("hw", [(8, 8), (35, 35), (8, 11)], ids=["8x8", "35x35", "8x11"])      # 8 x 11: rows and columns cannot be exchanged unnoticed
def test_pool3_against_fp64(hw):
    from mcvd_pytorch_amd import _lib
    H, W = hw
    gen = torch.Generator().manual_seed(H * W)
    x = torch.randn(2, 5, H, W, generator=gen)
    xc = x.cuda()
    y = torch.full_like(xc, float("nan"))
    _lib.check(_lib.lib.mcvd_op_pool3(_ctx().h, P(xc), P(y), 10, H, W, 0), "op_pool3")
    want = F.avg_pool2d(x.double(), kernel_size=3, stride=1, padding=1, count_include_pad=False)
    mag = F.avg_pool2d(x.double().abs(), kernel_size=3, stride=1, padding=1, count_include_pad=False)
    ratio = ((y.cpu().double() - want).abs() / mag).max().item() / 2.0 ** -22
    print(f"  avg pool {H} x {W}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0
    _lib.check(_lib.lib.mcvd_op_pool3(_ctx().h, P(xc), P(y), 10, H, W, 1), "op_pool3")
    assert torch.equal(y.cpu(), F.max_pool2d(x, kernel_size=3, stride=1, padding=1))


def test_global_average_within_one_ulp():
    from mcvd_pytorch_amd import _lib
    gen = torch.Generator().manual_seed(3)
    for hw in (64, 289):
        x = (torch.randn(3 * 100, hw, generator=gen) + 0.5)
        xc = x.cuda()
        y = torch.full((300,), float("nan"), device="cuda")
        _lib.check(_lib.lib.mcvd_op_global_avg(_ctx().h, P(xc), P(y), 300, hw), "op_global_avg")
        m64 = x.double().mean(1)
        m32 = m64.float()
        ulp = (torch.nextafter(m32.abs(), torch.tensor(float("inf"))) - m32.abs()).double()
        err = ((y.cpu().double() - m64).abs() / ulp).max().item()
        print(f"  global average over {hw}: worst error {err:.3f} ulp")
        assert err <= 1.0


@pytest.mark.parametrize("key", ["32", "64", "40x56", "299", "300"])
def test_resize_to_299_against_torchs_stored_values(golden_dir, key):
    from mcvd_pytorch_amd import _lib
    g = fixture(golden_dir)
    c = g["resize"][key]
    x = ir.make_images(g["seed"], c["name"], c["shape"])
    n, _, H, W = x.shape
    xc = x.expand(n, 3, H, W).contiguous().cuda()
    y = torch.full((n, 3, 299, 299), float("nan"), device="cuda")
    _lib.check(_lib.lib.mcvd_op_resize299(_ctx().h, P(xc), n, H, W, 1, P(y)), "op_resize299")
    y = y.cpu()
    rows = g["resize_stripe"]
    want_r, want_c = g[f"resize_rows_{key}"], g[f"resize_cols_{key}"]
    scale = max(want_r.abs().max().item(), want_c.abs().max().item())
    gate = GATE_FACTOR * c["rel_dev"]
    worst = 0.0
    for ch in range(3):
        worst = max(worst, (y[:, ch:ch + 1][:, :, rows] - want_r).abs().max().item() / scale,
                    (y[:, ch:ch + 1][:, :, :, rows] - want_c).abs().max().item() / scale)
    print(f"  resize {key}: deviation from torch {worst:.3e}, torch's own fp32 deviation {c['rel_dev']:.3e} (gate {GATE_FACTOR} x)")
    assert torch.isfinite(y).all() and worst <= gate
    if key == "299":
        assert torch.equal(y, 2 * x.expand(n, 3, H, W) - 1)
        plain = torch.empty_like(xc)
        _lib.check(_lib.lib.mcvd_op_resize299(_ctx().h, P(xc), n, H, W, 0, P(plain)), "op_resize299")
        assert torch.equal(plain, xc)


def test_every_block_of_the_fixture(golden_dir):
    """The fixture's weights and its six images (64 x 64, 40 x 56, 299 x 299): every block within 8 x its ref_rel_dev of the fp64
    restatement, block 3 as close to the real module's stored fp32 output as that implies."""
    g = fixture(golden_dir)
    det = detector(g["seed"], (0, 1, 2, 3))
    worst = [0.0] * 4
    for key, n in g["sets"]:
        out = det(images(g, key).cuda())
        want = restated(str(golden_dir), key, torch.float64)
        assert len(out) == 4
        for b in range(4):
            assert out[b].dtype == torch.float32 and out[b].shape == want[b].shape and torch.isfinite(out[b]).all()
            dev = ir.rel_dev(out[b].cpu(), want[b])
            worst[b] = max(worst[b], dev / g["ref_rel_dev"][b])
            assert dev <= GATE_FACTOR * g["ref_rel_dev"][b], (key, b, dev / g["ref_rel_dev"][b])
        real = g["block3"][key]
        # |device - real| <= |device - fp64| + |fp64 - real|
        assert (out[3].cpu() - real).abs().max().item() <= (GATE_FACTOR + 1) * g["ref_rel_dev"][3] * want[3].abs().max().item()
    print("  fid_inception: ratio to ref_rel_dev per block " + ", ".join(f"{r:.2f}" for r in worst) + f" (gate {GATE_FACTOR})")


def test_block3_alone_gives_the_same_bits(golden_dir):
    g = fixture(golden_dir)
    x = g["images_64"].cuda()
    full = detector(g["seed"], (0, 1, 2, 3))(x)
    only = detector(g["seed"], (3,))(x)
    assert len(only) == 1 and torch.equal(only[0], full[3])
    mid = detector(g["seed"], (1,))(x)
    assert len(mid) == 1 and torch.equal(mid[0], full[1])


def test_finalize_names_the_withheld_tensor(golden_dir):
    from mcvd_pytorch_amd import FidInception
    g = fixture(golden_dir)
    withheld = "Mixed_6c.branch7x7dbl_3.bn.running_mean"
    det = FidInception(device="cuda:0").load_state_dict({k: v for k, v in weights(g["seed"]).items() if k != withheld})
    with pytest.raises(RuntimeError, match=rf"code {ESTATE}\).*missing {withheld}"):
        det(g["images_64"].cuda())
    det.load_state_dict({withheld: weights(g["seed"])[withheld]})
    assert torch.equal(det(g["images_64"].cuda())[0], detector(g["seed"], (3,))(g["images_64"].cuda())[0])


def test_load_state_dict_and_call_errors(golden_dir):
    from mcvd_pytorch_amd import FidInception
    g = fixture(golden_dir)
    sd = weights(g["seed"])
    det = FidInception(device="cuda:0")
    det.load_state_dict({"fc.weight": torch.zeros(1008, 2048), "AuxLogits.conv0.conv.weight": torch.zeros(1),
                         "Conv2d_1a_3x3.bn.num_batches_tracked": torch.tensor(0)})
    with pytest.raises(ValueError, match="unknown key"):
        det.load_state_dict({"Mixed_8a.branch1x1.conv.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match="shape"):
        det.load_state_dict({"Mixed_6b.branch7x7_2.conv.weight": sd["Mixed_6b.branch7x7_3.conv.weight"]})
    with pytest.raises(ValueError, match="3 channels"):
        detector(g["seed"], (3,))(torch.zeros(2, 1, 32, 32, device="cuda"))
    fixed = FidInception(resize_input=False, device="cuda:0")
    with pytest.raises(ValueError, match="299 x 299"):
        fixed(torch.zeros(1, 3, 64, 64, device="cuda"))
    with pytest.raises(ValueError, match="output_blocks"):
        FidInception(output_blocks=(4,), device="cuda:0")


def test_chunk_and_batch_invariance(golden_dir):
    """Chunk size + 1 images of 32 x 32: each image's 2048 features are the same bits alone, in a batch of 5 and in the whole batch (which
    spans two chunks)."""
    from mcvd_pytorch_amd import _lib
    g = fixture(golden_dir)
    det = detector(g["seed"], (3,))
    n = _lib.lib.mcvd_inception_chunk() + 1
    assert n >= 17
    x = ir.make_images(g["seed"], "invariance", (n, 3, 32, 32)).cuda()
    whole = det(x)[0]
    assert whole.shape == (n, 2048, 1, 1)
    for i in range(n):
        assert torch.equal(det(x[i:i + 1])[0][0], whole[i]), i
    for i in (0, 6, n - 5):
        assert torch.equal(det(x[i:i + 5])[0], whole[i:i + 5]), i
    assert (whole[0] - whole[1]).abs().max().item() > 0


def test_existing_callers_take_the_detector(golden_dir):
    """fid_pr and NearestNeighbors with FidInception as `detector=` equal the same calls on the features of detector(x)[0]."""
    from mcvd_pytorch_amd import NearestNeighbors, fid_pr, knn_search
    from mcvd_pytorch_amd.metrics import hflip_u8
    g = fixture(golden_dir)
    det = detector(g["seed"], (3,))
    real = ir.make_images(g["seed"], "callers_real", (8, 3, 32, 32)).cuda()
    fake = ir.make_images(g["seed"], "callers_fake", (8, 3, 32, 32)).cuda()
    fr, ff = det(real)[0].reshape(8, -1), det(fake)[0].reshape(8, -1)
    got = fid_pr(real, fake, detector=det, k=3)
    want = fid_pr(fr, ff, k=3)
    assert got == want and all(torch.isfinite(torch.as_tensor(v)).all() for v in got)
    nn = NearestNeighbors(fake, det, k=3, n_samples=8)
    nn.update(real)
    res = nn.result()
    _, index = knn_search(ff, fr, k=3, query2=det(hflip_u8(fake))[0].reshape(8, -1))
    assert torch.equal(res["indices"], index)
