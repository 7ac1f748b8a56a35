"""CPU restatement of video_gen's test-mode metrics (runners/ncsn_runner.py:1580-1609, :1749-1778, :2195-2255) in torch float64, with
no scipy, no PIL and no skimage, so that it runs wherever the tests run.  The tests check it against scipy / Pillow where those exist and
against the fixtures recorded from the real runner.

Per (video, frame), on pred / real [B, T*C, H, W] in [0, 1]:
  1. mse: F.mse_loss(real_ij, pred_ij) in fp32 (frame_mse); frame_mse64 is the fp64 mean of the same fp32 differences.
  2. quantisation: torchvision to_pil_image of a float tensor = pic.mul(255).byte() (one fp32 multiply, truncation).
  3. grey: .convert("RGB").convert("L") = Pillow's luma (19595 R + 38470 G + 7471 B + 0x8000) >> 16 (C = 3); an L image maps to itself.
  4. MNIST rule: torch.round (half to even) before 2-3.
  5. ssim: skimage.metrics.structural_similarity(p, r, data_range=255, gaussian_weights=True, use_sample_covariance=False), restated
     from skimage >= 0.19's algorithm for 2-D input: float64 images; scipy.ndimage.gaussian_filter(., sigma=1.5, truncate=3.5) of
     X, Y, X^2, Y^2, XY (weights exp(-x^2 / (2 sigma^2)) normalised, x = -5..5); v = E[.^2] - E[.]^2 (covariance norm 1);
     C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2; S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)); the mean of S
     over the interior with a 5-pixel border cropped.  The interior reads no pixel outside the frame, so the filter's border mode
     does not matter and the moments are computed on the valid region only.
  6. per video: vid_mse = fp32 sum of the frame MSEs in frame order / T; vid_ssim = the same with Python floats.
  7. summary: best of preds_per_test consecutive rows; mean, std (ddof 0) and conf95 = avg - norm.interval(0.95, avg, sem)[0], with
     the normal quantile from the standard library (statistics.NormalDist) instead of scipy.

skimage itself is not installed where these fixtures were made, so step 5 was never compared with skimage; it is written so that a reader
can check it against skimage's source (skimage/metrics/_structural_similarity.py).
"""
import math
import statistics

import numpy as np
import torch
import torch.nn.functional as F

SIGMA, RADIUS = 1.5, 5
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
MNIST = ("STOCHASTICMOVINGMNIST", "MOVINGMNIST")


def gauss_taps():
    x = torch.arange(-RADIUS, RADIUS + 1, dtype=torch.float64)
    phi = torch.exp(-0.5 / (SIGMA * SIGMA) * x ** 2)
    return phi / phi.sum()


def luma(r, g, b):
    """Pillow's RGB -> L conversion on integer tensors."""
    return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16


def grey_planes(x01, channels, binary=False):
    """[B, T*C, H, W] fp32 in [0, 1] -> [B, T, H, W] uint8 as np.asarray(ToPILImage()(frame).convert("RGB").convert("L"))."""
    x = x01.detach().cpu().float()
    if binary:
        x = torch.round(x)
    q = x.mul(255).byte()
    B, TC, H, W = q.shape
    q = q.reshape(B, TC // channels, channels, H, W).long()
    if channels == 1:
        return q[:, :, 0].to(torch.uint8)
    if channels == 3:
        return luma(q[:, :, 0], q[:, :, 1], q[:, :, 2]).to(torch.uint8)
    raise ValueError(f"{channels} channels")


def moments(a):
    """Gaussian-filtered moments on the interior: a [N, H, W] float64 -> [N, H-10, W-10] (filter along H, then along W)."""
    w = gauss_taps()
    x = a[:, None]
    x = F.conv2d(x, w.view(1, 1, -1, 1))
    x = F.conv2d(x, w.view(1, 1, 1, -1))
    return x[:, 0]


def ssim_planes(p, r):
    """Per-plane SSIM of uint8 planes [N, H, W] -> float64 [N]."""
    if p.shape[-1] < 2 * RADIUS + 1 or p.shape[-2] < 2 * RADIUS + 1:
        raise ValueError("win_size exceeds image extent")
    X, Y = p.double(), r.double()
    ux, uy, uxx, uyy, uxy = (moments(v) for v in (X, Y, X * X, Y * Y, X * Y))
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    return S.flatten(1).mean(1)


def frame_mse(pred01, real01, channels):
    """F.mse_loss(real_ij, pred_ij) per frame, fp32 [B, T] (the reference's own call)."""
    B, TC = pred01.shape[:2]
    out = torch.empty(B, TC // channels)
    for b in range(B):
        for t in range(TC // channels):
            sl = slice(t * channels, (t + 1) * channels)
            out[b, t] = F.mse_loss(real01[b, sl].cpu().float(), pred01[b, sl].cpu().float())
    return out


def frame_mse64(pred01, real01, channels):
    """fp64 mean of the fp32 differences real - pred per frame, [B, T] float64."""
    d = (real01.cpu().float() - pred01.cpu().float()).double()
    B, TC, H, W = d.shape
    return (d * d).reshape(B, TC // channels, -1).mean(-1)


def frame_metrics(pred01, real01, channels, binary=False):
    """-> (mse fp32 [B, T], ssim fp64 [B, T], grey_pred [B, T, H, W], grey_real)."""
    gp, gr = grey_planes(pred01, channels, binary), grey_planes(real01, channels, binary)
    B, T, H, W = gp.shape
    s = ssim_planes(gp.reshape(B * T, H, W), gr.reshape(B * T, H, W)).reshape(B, T)
    return frame_mse(pred01, real01, channels), s, gp, gr


def video_values(mse_bt, ssim_bt):
    """Steps 6: per-video values as the reference accumulates them (0-dim fp32 tensors; Python floats)."""
    vm, vs = [], []
    for b in range(mse_bt.shape[0]):
        m, s = 0, 0
        for t in range(mse_bt.shape[1]):
            m = m + mse_bt[b, t].float()
            s = s + float(ssim_bt[b, t])
        vm.append(m / mse_bt.shape[1])
        vs.append(s / mse_bt.shape[1])
    return vm, vs


def _stats(metric):
    avg, std = metric.mean().item(), metric.std().item()
    n = len(metric)
    sem = float(np.std(metric, ddof=1) / n ** 0.5) if n > 1 else math.nan
    if not (sem > 0) or avg != avg:
        return avg, std, math.nan
    z = statistics.NormalDist().inv_cdf((1.0 - 0.95) / 2)
    return avg, std, avg - (z * sem + avg)


def summary(vid_mse, vid_ssim, ppt, suffix=""):
    """Step 7 for one phase's lists: {mse, mse_std, mse_conf95, psnr..., ssim...} with `suffix` after the metric name."""
    m = np.array([float(v) for v in vid_mse], dtype=np.float32) if all(torch.is_tensor(v) for v in vid_mse) else np.array(vid_mse)
    with np.errstate(divide="ignore"):
        lists = {"mse": m.reshape(-1, ppt).min(-1), "psnr": (10 * np.log10(1 / m)).reshape(-1, ppt).max(-1),
                 "ssim": np.array(vid_ssim).reshape(-1, ppt).max(-1)}
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, v in lists.items():
            out[f"{k}{suffix}"], out[f"{k}{suffix}_std"], out[f"{k}{suffix}_conf95"] = _stats(v)
    return out
