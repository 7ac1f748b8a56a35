"""CPU restatement of video_gen's LPIPS (runners/ncsn_runner.py:1427-1431, :1590-1591, :1602-1609, :2199-2215; models/networks_basic.py:25-97,
models/pretrained_networks.py:56-94, models/eval_models.py:35-37) in integers and torch float64, with no PIL and no torchvision, so that it
runs wherever the tests run.  Besides the kernels (csrc/kernels/lpips.cpp) this is the one place the algorithm is written down.

Per (video, frame), on pred / real [B, T*C, H, W] fp32 in [0, 1]:
  1. quantisation: ToPILImage() = pic.mul(255).byte().  NO MNIST rounding here: LPIPS takes the un-rounded frame for every dataset.
  2. .convert("RGB"): C = 1 replicates the plane, C = 3 is the identity.
  3. Resize((128, 128)) = Pillow's Image.resize(BILINEAR) on uint8: a horizontal pass, then a vertical pass over its uint8 result; a pass
     whose input and output length agree is skipped.  Per pass and output index xx (Pillow's precompute_coeffs / normalize_coeffs_8bpc,
     all in double): scale = in / out; fs = max(scale, 1); support = 1.0 * fs; center = (xx + 0.5) * scale;
     xmin = max(int(center - support + 0.5), 0); xmax = min(int(center + support + 0.5), in); the taps
     w[x] = triangle((x + xmin - center + 0.5) / fs), x < xmax - xmin, divided by their sum, then int(0.5 + w * 2^22); the output is
     clip((2^21 + sum_x u8[xmin + x] * k[x]) >> 22, 0, 255).
  4. ToTensor (u8 / 255) and Normalize(0.5, 0.5) ((x - 0.5) / 0.5), both in fp32 as torchvision does them.
  5. PNetLin v0.1 in eval mode, here in fp64: (x - shift) / scale; AlexNet `features` with a tap behind each of the five ReLUs; per tap
     f / (sqrt(sum_c f^2) + 1e-10), the squared difference of the two images' unit features, the tap's lin weights as a dot over
     channels, the spatial mean; the five values added in tap order.
  6. per video: the fp32 frame values added in frame order as fp32 tensors, then float(.) / T.
  7. summary: min over preds_per_test consecutive rows, then mean / std / conf95 as tests/metrics_ref.py does for the other metrics.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import synth
from tests import metrics_ref

SIZE = 128
PRECISION_BITS = 32 - 8 - 2
CHNS = (64, 192, 384, 256, 256)
# (torchvision features index, reference slice name, Cout, Cin, ks, stride, pad)
CONVS = ((0, "slice1.0", 64, 3, 11, 4, 2), (3, "slice2.3", 192, 64, 5, 1, 2), (6, "slice3.6", 384, 192, 3, 1, 1),
         (8, "slice4.8", 256, 384, 3, 1, 1), (10, "slice5.10", 256, 256, 3, 1, 1))
POOL_BEFORE = (False, True, True, False, False)      # MaxPool2d(3, 2) in front of the conv
RECIPE = "randn*sqrt(2/fan_in); bias 0.1*randn; generator oracle.synth._gen(seed, 'features.N.weight|bias')"


def make_backbone(seed):
    """Seeded stand-in for torchvision's AlexNet `features` state dict (keys features.N.weight / bias): one generator per tensor."""
    sd = {}
    for idx, _, cout, cin, ks, _, _ in CONVS:
        fan_in = cin * ks * ks
        sd[f"features.{idx}.weight"] = torch.randn((cout, cin, ks, ks), generator=synth._gen(seed, f"features.{idx}.weight")) * (2.0 / fan_in) ** 0.5
        sd[f"features.{idx}.bias"] = 0.1 * torch.randn((cout,), generator=synth._gen(seed, f"features.{idx}.bias"))
    return sd


def backbone_probe(sd):
    """name -> (fp64 sum, 64 probed values at fixed strides): what the fixtures store instead of the 9.9 MB of weights."""
    out = {}
    for k, v in sd.items():
        flat = v.reshape(-1)
        idx = torch.linspace(0, flat.numel() - 1, 64).long()
        out[k] = (float(flat.double().sum()), flat[idx].clone())
    return out


@functools.lru_cache(maxsize=None)
def resize_coeffs(in_size, out_size=SIZE):
    """Pillow's bilinear tables for one axis -> (xmin [out] int, n [out] int, k [out, ksize] int64)."""
    scale = in_size / out_size
    fs = scale if scale >= 1.0 else 1.0
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    xmin_a, n_a, k_a = np.zeros(out_size, np.int64), np.zeros(out_size, np.int64), np.zeros((out_size, ksize), np.int64)
    ss = 1.0 / fs
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w, ww = [], 0.0
        for x in range(xmax):
            a = (x + xmin - center + 0.5) * ss
            a = -a if a < 0.0 else a
            v = 1.0 - a if a < 1.0 else 0.0
            w.append(v)
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            k_a[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        xmin_a[xx], n_a[xx] = xmin, xmax
    return xmin_a, n_a, k_a


def _resample_last(a, out_size):
    """One pass along the last axis of an integer array of uint8 values."""
    in_size = a.shape[-1]
    if in_size == out_size:
        return a
    xmin, n, k = resize_coeffs(in_size, out_size)
    idx = np.minimum(xmin[:, None] + np.arange(k.shape[1])[None, :], in_size - 1)      # taps beyond n carry a zero coefficient
    acc = (a[..., idx].astype(np.int64) * k).sum(-1) + (1 << (PRECISION_BITS - 1))
    return np.clip(acc >> PRECISION_BITS, 0, 255)


def resize_u8(planes, out_size=SIZE):
    """uint8 planes [..., H, W] -> [..., out, out] as PIL's Image.resize((out, out), BILINEAR): horizontal, then vertical."""
    a = np.asarray(planes).astype(np.int64)
    a = _resample_last(a, out_size)
    a = np.swapaxes(_resample_last(np.swapaxes(a, -1, -2), out_size), -1, -2)
    return a.astype(np.uint8)


def quantise(x01):
    return x01.detach().cpu().float().mul(255).byte()


def resized_planes(x01, channels):
    """[B, T*C, H, W] fp32 -> uint8 [B, T, C, 128, 128] (steps 1 and 3; step 2's replication is left to net_input)."""
    q = quantise(x01)
    B, TC, H, W = q.shape
    return torch.from_numpy(resize_u8(q.numpy())).reshape(B, TC // channels, channels, SIZE, SIZE)


def net_input(planes_u8):
    """uint8 [N, C, 128, 128] -> fp32 [N, 3, 128, 128] in [-1, 1] (steps 2 and 4, torchvision's fp32 arithmetic)."""
    if planes_u8.shape[1] == 1:
        planes_u8 = planes_u8.expand(-1, 3, -1, -1)
    elif planes_u8.shape[1] != 3:
        raise ValueError(f"{planes_u8.shape[1]} channels")
    x = planes_u8.to(torch.float32).div(255)
    return x.sub(0.5).div(0.5)


def taps(x, backbone, shift, scale, dtype=torch.float64):
    """The five post-ReLU feature maps of [N, 3, 128, 128] images in `dtype`."""
    h = (x.to(dtype) - shift.to(dtype).reshape(1, 3, 1, 1)) / scale.to(dtype).reshape(1, 3, 1, 1)
    out = []
    for (idx, _, _, _, _, stride, pad), pool in zip(CONVS, POOL_BEFORE):
        if pool:
            h = F.max_pool2d(h, 3, 2)
        h = F.relu(F.conv2d(h, backbone[f"features.{idx}.weight"].to(dtype), backbone[f"features.{idx}.bias"].to(dtype), stride=stride, padding=pad))
        out.append(h)
    return out


def distance(taps0, taps1, lins):
    """-> (value [N], per tap [N, 5]) in the taps' dtype; lins: five [C_k] weight vectors."""
    per = []
    for f0, f1, w in zip(taps0, taps1, lins):
        u0 = f0 / (torch.sqrt((f0 ** 2).sum(1, keepdim=True)) + 1e-10)
        u1 = f1 / (torch.sqrt((f1 ** 2).sum(1, keepdim=True)) + 1e-10)
        d = ((u0 - u1) ** 2 * w.to(f0.dtype).reshape(1, -1, 1, 1)).sum(1)
        per.append(d.mean((1, 2)))
    per = torch.stack(per, 1)
    val = per[:, 0].clone()
    for k in range(1, per.shape[1]):
        val = val + per[:, k]
    return val, per


def frame_lpips64(pred01, real01, channels, backbone, lins, shift, scale, chunk=16):
    """Steps 1-5 -> (value [B, T] fp64, per tap [B, T, 5] fp64, resized uint8 planes [2, B, T, C, 128, 128] (pred, then real))."""
    rp, rr = resized_planes(pred01, channels), resized_planes(real01, channels)
    B, T = rp.shape[:2]
    p, r = rp.reshape(B * T, channels, SIZE, SIZE), rr.reshape(B * T, channels, SIZE, SIZE)
    vals, pers = [], []
    for i in range(0, B * T, chunk):
        tp = taps(net_input(p[i:i + chunk]), backbone, shift, scale)
        tr = taps(net_input(r[i:i + chunk]), backbone, shift, scale)
        v, per = distance(tp, tr, lins)
        vals.append(v)
        pers.append(per)
    return torch.cat(vals).reshape(B, T), torch.cat(pers).reshape(B, T, 5), torch.stack([rp, rr])


def video_lpips(lpips_bt):
    """Step 6: avg_distance = 0; avg_distance += fp32 tensor per frame; avg_distance.item() / T."""
    x = torch.as_tensor(lpips_bt).cpu().float()
    out = []
    for b in range(x.shape[0]):
        s = 0
        for t in range(x.shape[1]):
            s = s + x[b, t]
        out.append(s.item() / x.shape[1])
    return out


def summary(vid_lpips, ppt, suffix=""):
    """Step 7 for one phase's list: {lpips, lpips_std, lpips_conf95} with `suffix` after the metric name."""
    arr = np.array(vid_lpips).reshape(-1, ppt).min(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        avg, std, c95 = metrics_ref._stats(arr)
    return {f"lpips{suffix}": avg, f"lpips{suffix}_std": std, f"lpips{suffix}_conf95": c95}
