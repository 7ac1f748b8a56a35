"""The numbers video_gen's test mode reports per phase: MSE, PSNR, SSIM, LPIPS and FVD (runners/ncsn_runner.py:1580-1609, :1749-1778,
:1918-1982, :2195-2278), with the per-frame work on the device (mcvd_frame_metrics, kernels/metrics.cpp; mcvd_lpips_frames,
kernels/lpips.cpp; mcvd_fvd_clips and mcvd_feature_stats, kernels/fvd.cpp) and the per-video / summary arithmetic on the host in the
reference's dtypes and order.

LPIPS (v0.1, AlexNet, "net-lin") is computed when the caller hands VideoMetrics an LpipsNet that holds the weights: the backbone is
torchvision's AlexNet `features` state dict and the five lin layers are the reference's models/weights/v0.1/alex.pth, both supplied by the
caller as a MCVD checkpoint is -- the package ships no weights, downloads none and has no default.  The ScalingLayer's six constants are
part of the architecture (models/networks_basic.py:93-94) and are set at construction.

FVD is computed when the caller hands VideoMetrics the detector as a callable (`fvd=`): the reference's I3D is a TorchScript file
(models/fvd/fvd.py:30-38), not an architecture one can restate, so the package holds no detector, ships none and downloads none -- the
caller brings `torch.jit.load(...)` of that file on the GPU, or any callable of the same call shape.  Everything around that one call is
here: the gates (fvd_gates), the clip assembly and preprocess_single on the device (fvd_clips), the batching in tens, the fp64 feature
statistics on the device (feature_stats), the Frechet distance (frechet_distance), the per-trajectory values and the three key groups.

fast_fid's scores (evaluation/fid_PR.py, NCSNRunner.fast_fid) are at the end of the module: FID from the same feature_stats /
frechet_from_stats, and the improved precision and recall (k-nearest-neighbour manifolds) in fp64 on the device without the pairwise
distance matrices (mcvd_knn_radii, mcvd_manifold_hits, kernels/prdc.cpp).  `detector=` takes any callable; the reference's own detector,
the FID InceptionV3 of evaluation/inception.py, is FidInception below (mcvd_inception_*, kernels/inception.cpp): the architecture runs on
the device and the caller hands over the weights (pt_inception-2015-12-05-6726825d.pth) as a state dict or a path -- the package holds
none and downloads none, as with LPIPS.

Deliberate divergences from the reference:
  * frames of 2 or 4 channels (torchvision's LA / RGBA images) are refused with ValueError: no MCVD dataset has them;
  * :1742-1747: phase (2) tests phase (1)'s `real` / `pred` shapes and, when it cannot compute, appends its zeros to phase (1)'s lists.
    Here phase (2) tests its own frames and appends to its own lists;
  * :2222: the per-trajectory FVDs are taken in the order np.random.choice(arange(ppt), (ppt,), replace=False) draws -- a permutation of
    all of them, of which mean, std and sem do not depend beyond rounding.  Here they are taken in order 0 .. ppt - 1 and numpy's global
    RNG is not touched;
  * frechet_distance takes tr sqrtm(S_g S_r) as the sum of Re sqrt(lambda_i) over the eigenvalues of the product (no scipy): 1e-14 .. 1e-12
    relative to the reference's scipy route where both covariances have full rank, 1e-9 where they are singular (rows <= d), where
    scipy's sqrtm is itself only defined to about sqrt(eps).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib

# scipy.stats.norm.interval(0.95)[0] is ndtri((1.0 - 0.95) / 2) = ndtri(0.025000000000000022); the literal differs from ndtri(0.025)
# in its last bit.  Kept as a constant so that scipy is not a dependency (tests check it against scipy.special.ndtri where installed).
_NDTRI_Q1 = float.fromhex("-0x1.f5c0331eeff84p+0")
_MNIST = ("STOCHASTICMOVINGMNIST", "MOVINGMNIST")

_ctxs = {}   # device index -> the package's own context (frame_metrics without a scorenet); lives until the process exits


def _package_ctx(device):
    ctx = _ctxs.get(device.index)
    if ctx is None:
        ctx = C.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib.mcvd_ctx_create(device.index, C.c_void_p(torch.cuda.current_stream(device).cuda_stream), C.byref(ctx)),
                       "ctx_create")
        _ctxs[device.index] = ctx
    # bound to torch's current stream on every call: a context on the same stream as a HipScoreNet's does not count as sharing the device
    _lib.check(_lib.lib.mcvd_ctx_set_stream(ctx, C.c_void_p(torch.cuda.current_stream(device).cuda_stream)), "ctx_set_stream")
    return ctx


@torch.no_grad()
def frame_metrics(pred01, real01, channels, binary=False, scorenet=None, return_grey=False):
    """Per-frame MSE and SSIM of [B, T*C, H, W] frames in [0, 1] (inverse_data_transform's output) -> (mse [B, T] float32,
    ssim [B, T] float64) on the device: the inner loop of runners/ncsn_runner.py:1580-1609.

      * mse: F.mse_loss(real_ij, pred_ij) -- the fp32 differences, squared and summed in fp64, rounded to fp32 once;
      * ssim: skimage structural_similarity(data_range=255, gaussian_weights=True, use_sample_covariance=False) of the grey planes
        np.asarray(ToPILImage()(x).convert("RGB").convert("L")); `binary` (the MNIST rule, :1596-1599) torch.round()s both frames first.

    With `scorenet` the work runs on that net's context and stream (as frames_to_uint8); without, on a context of this module bound to
    torch's current stream.  `return_grey=True` also returns the uint8 grey planes [2, B, T, H, W] (pred, then real)."""
    if channels not in (1, 3):
        raise ValueError(f"frame_metrics: {channels}-channel frames are not supported (1 = L or 3 = RGB; torchvision's LA / RGBA images "
                         "of 2 / 4 channels are refused deliberately)")
    dev = scorenet.device if scorenet is not None else (pred01.device if pred01.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    p = pred01.to(device=dev, dtype=torch.float32).contiguous()
    r = real01.to(device=dev, dtype=torch.float32).contiguous()
    if p.dim() != 4 or p.shape != r.shape:
        raise ValueError(f"frame_metrics: pred {tuple(p.shape)} and real {tuple(r.shape)} must be the same [B, T*C, H, W]")
    B, TC, H, W = p.shape
    if TC % channels:
        raise ValueError(f"{TC} channels is not a multiple of {channels}")
    if H < 11 or W < 11:
        raise ValueError(f"frame_metrics: a {H} x {W} frame is smaller than the 11 x 11 SSIM window (skimage raises here too)")
    T = TC // channels
    mse = torch.empty((B, T), dtype=torch.float32, device=dev)
    ssim = torch.empty((B, T), dtype=torch.float64, device=dev)
    grey = torch.empty((2, B, T, H, W), dtype=torch.uint8, device=dev) if return_grey else None
    with torch.cuda.device(dev):
        if scorenet is not None:
            scorenet._bind_stream()
            ctx = scorenet._ctx
        else:
            ctx = _package_ctx(dev)
        _lib.check(_lib.lib.mcvd_frame_metrics(ctx, C.c_void_p(p.data_ptr()), C.c_void_p(r.data_ptr()), B, T, channels, H, W,
                                               _lib.METRIC_ROUND_BINARY if binary else 0, C.c_void_p(mse.data_ptr()),
                                               C.c_void_p(ssim.data_ptr()), C.c_void_p(grey.data_ptr() if grey is not None else None)),
                   "frame_metrics")
    return (mse, ssim, grey) if return_grey else (mse, ssim)


def video_values(mse_bt, ssim_bt):
    """Per-frame values [B, T] (host arrays or tensors) -> (vid_mse, vid_ssim) lists of the reference's per-video values (:1605-1607):
    vid_mse = (sum of the fp32 frame MSEs, in frame order, from 0) / T in fp32; vid_ssim = the same with Python floats."""
    mse_bt = np.asarray(torch.as_tensor(mse_bt).cpu(), dtype=np.float32)
    ssim_bt = np.asarray(torch.as_tensor(ssim_bt).cpu(), dtype=np.float64)
    T = mse_bt.shape[1]
    vid_mse, vid_ssim = [], []
    for b in range(mse_bt.shape[0]):
        m, s = mse_bt[b, 0], 0.0 + float(ssim_bt[b, 0])
        for t in range(1, T):
            m = np.float32(m + mse_bt[b, t])
            s += float(ssim_bt[b, t])
        vid_mse.append(np.float32(m / np.float32(T)))
        vid_ssim.append(s / T)
    return vid_mse, vid_ssim


def image_metric_stuff(metric):
    """(mean, std, conf95) of one metric array as :2201-2204 computes them: numpy mean / std (ddof 0), and
    conf95 = avg - norm.interval(0.95, loc=avg, scale=sem(metric))[0] with sem = std(ddof=1) / sqrt(n) in the array's dtype and
    scipy's ppf rules (nan where the scale is not > 0 or the location is nan)."""
    metric = np.asarray(metric)
    avg, std = metric.mean().item(), metric.std().item()
    with np.errstate(invalid="ignore", divide="ignore"):
        sem = np.std(metric, ddof=1) / len(metric) ** 0.5
    scale = np.float64(sem)
    lo = _NDTRI_Q1 * scale + avg if (scale > 0 and avg == avg) else math.nan
    return avg, std, avg - float(lo)


def summarize(vid_mse, vid_ssim, preds_per_test=1, suffix=""):
    """The reference's per-phase summary (:2195-2215, :2241-2255): best of `preds_per_test` consecutive rows (min MSE, max PSNR,
    max SSIM), then image_metric_stuff of each list.  Keys mse, mse_std, mse_conf95, psnr..., ssim... with `suffix` after the metric
    name ("2" for phase (2): mse2, mse2_std, ...)."""
    with np.errstate(divide="ignore"):
        mse_list = np.array(vid_mse).reshape(-1, preds_per_test).min(-1)
        psnr_list = (10 * np.log10(1 / np.array(vid_mse))).reshape(-1, preds_per_test).max(-1)
    ssim_list = np.array(vid_ssim).reshape(-1, preds_per_test).max(-1)
    out = {}
    for name, arr in (("mse", mse_list), ("psnr", psnr_list), ("ssim", ssim_list)):
        avg, std, c95 = image_metric_stuff(arr)
        out[f"{name}{suffix}"], out[f"{name}{suffix}_std"], out[f"{name}{suffix}_conf95"] = avg, std, c95
    return out


_LPIPS_CONVS = ((0, "slice1"), (3, "slice2"), (6, "slice3"), (8, "slice4"), (10, "slice5"))


class _DeviceNet:
    """What LpipsNet and FidInception share: a net object of the library (mcvd_<_KIND>_create / _set_param / _finalize / _destroy) on a
    scorenet's context and stream, or on this module's own context."""
    _KIND = None

    @classmethod
    def _require_gpu(cls):
        if not torch.cuda.is_available():
            raise RuntimeError(f"{cls.__name__} needs a ROCm GPU (MI355X); there is no CPU fallback")

    def __init__(self, device=None, scorenet=None):
        self._require_gpu()
        self.scorenet = scorenet
        if scorenet is not None:
            self.device = scorenet.device
        else:
            dev = torch.device(device if device is not None else "cuda")
            self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self._net = C.c_void_p()
        self._final = False
        with torch.cuda.device(self.device):
            _lib.check(getattr(_lib.lib, f"mcvd_{self._KIND}_create")(self._ctx(), C.byref(self._net)), f"{self._KIND}_create")

    def _ctx(self):
        if self.scorenet is not None:
            self.scorenet._bind_stream()
            return self.scorenet._ctx
        return _package_ctx(self.device)

    def _set(self, name, t):
        t = t.detach().to(device="cpu", dtype=torch.float32).contiguous()
        shape = (C.c_int64 * t.dim())(*t.shape)
        _lib.check(getattr(_lib.lib, f"mcvd_{self._KIND}_set_param")(self._net, name.encode(), C.c_void_p(t.data_ptr()), shape, t.dim(), 0),
                   f"{self._KIND}_set_param({name})")
        self._final = False

    def finalize(self):
        if not self._final:
            with torch.cuda.device(self.device):
                self._ctx()
                _lib.check(getattr(_lib.lib, f"mcvd_{self._KIND}_finalize")(self._net), f"{self._KIND}_finalize")
            self._final = True
        return self

    def __del__(self):
        try:
            if getattr(self, "_net", None):
                getattr(_lib.lib, f"mcvd_{self._KIND}_destroy")(self._net)
                self._net = None
        except Exception:
            pass


class LpipsNet(_DeviceNet):
    """The reference's eval_models.PerceptualLoss(model='net-lin', net='alex') (version 0.1, eval mode) on the device.

        net = LpipsNet(scorenet=hipnet)                       # or LpipsNet(device="cuda:0")
        net.load_backbone(torchvision_alexnet_state_dict)     # keys features.N.weight / bias; classifier keys are ignored
        net.load_linear("weights/v0.1/alex.pth")              # the reference's lin layers (path or state dict)
        # or net.load_state_dict(pnetlin.state_dict()) for a whole PNetLin dict

    Runs on the scorenet's context and stream when given one, else on this module's own context (as frame_metrics).  Missing weights are
    an error at the first use (MCVD_ESTATE names the tensor)."""

    _KIND = "lpips"

    def __init__(self, device=None, scorenet=None):
        super().__init__(device, scorenet)
        # ScalingLayer (models/networks_basic.py:93-94): constants of the architecture, not learned weights
        self._set("scaling_layer.shift", torch.tensor([-.030, -.088, -.188]))
        self._set("scaling_layer.scale", torch.tensor([.458, .448, .450]))

    def load_backbone(self, state_dict):
        for idx, _ in _LPIPS_CONVS:
            for kind in ("weight", "bias"):
                self._set(f"features.{idx}.{kind}", state_dict[f"features.{idx}.{kind}"])
        return self

    def load_linear(self, path_or_state_dict):
        sd = path_or_state_dict
        if not isinstance(sd, dict):
            sd = torch.load(sd, map_location="cpu")
        for k in range(5):
            self._set(f"lin{k}.model.1.weight", sd[f"lin{k}.model.1.weight"])
        for name in ("scaling_layer.shift", "scaling_layer.scale"):
            if name in sd:
                self._set(name, sd[name])
        return self

    def load_state_dict(self, sd):
        for name, t in sd.items():
            self._set(name, t)
        return self


@torch.no_grad()
def frame_lpips(pred01, real01, channels, net, return_taps=False):
    """Per-frame LPIPS of [B, T*C, H, W] frames in [0, 1] -> [B, T] float32 on the device: the `T2(...)` / `model_lpips.forward(real, pred)`
    lines of runners/ncsn_runner.py:1602-1605 for every frame at once.  The frames are NOT rounded under the MNIST rule (the reference
    rounds the SSIM planes only).  `return_taps=True` also returns the per-tap values [B, T, 5] and the resized uint8 planes
    [2, B, T, C, 128, 128] (pred, then real)."""
    if channels not in (1, 3):
        raise ValueError(f"frame_lpips: {channels}-channel frames are not supported (1 = L or 3 = RGB)")
    dev = net.device
    p = pred01.to(device=dev, dtype=torch.float32).contiguous()
    r = real01.to(device=dev, dtype=torch.float32).contiguous()
    if p.dim() != 4 or p.shape != r.shape:
        raise ValueError(f"frame_lpips: pred {tuple(p.shape)} and real {tuple(r.shape)} must be the same [B, T*C, H, W]")
    B, TC, H, W = p.shape
    if TC % channels:
        raise ValueError(f"{TC} channels is not a multiple of {channels}")
    T = TC // channels
    net.finalize()
    out = torch.empty((B, T), dtype=torch.float32, device=dev)
    taps = torch.empty((B, T, 5), dtype=torch.float32, device=dev) if return_taps else None
    planes = torch.empty((2, B, T, channels, 128, 128), dtype=torch.uint8, device=dev) if return_taps else None
    with torch.cuda.device(dev):
        net._ctx()
        _lib.check(_lib.lib.mcvd_lpips_frames(net._net, C.c_void_p(p.data_ptr()), C.c_void_p(r.data_ptr()), B, T, channels, H, W,
                                              C.c_void_p(out.data_ptr()), C.c_void_p(planes.data_ptr() if return_taps else None),
                                              C.c_void_p(taps.data_ptr() if return_taps else None)), "lpips_frames")
    return (out, taps, planes) if return_taps else out


def video_lpips(lpips_bt):
    """Per-frame values [B, T] -> the reference's per-video list (:1582, :1605, :1609): avg_distance = 0 + the fp32 frame values added in
    frame order as fp32, then .item() / T in Python floats."""
    x = np.asarray(torch.as_tensor(lpips_bt).cpu(), dtype=np.float32)
    T = x.shape[1]
    out = []
    for b in range(x.shape[0]):
        s = x[b, 0]
        for t in range(1, T):
            s = np.float32(s + x[b, t])
        out.append(float(s) / T)
    return out


def summarize_lpips(vid_lpips, preds_per_test=1, suffix=""):
    """The lpips keys of the reference's summary (:2199, :2209, :2215; :2245-2255 with suffix "2"): min over `preds_per_test` rows."""
    avg, std, c95 = image_metric_stuff(np.array(vid_lpips).reshape(-1, preds_per_test).min(-1))
    return {f"lpips{suffix}": avg, f"lpips{suffix}_std": std, f"lpips{suffix}_conf95": c95}


def fvd_gates(config):
    """(calc_fvd1, calc_fvd2, calc_fvd3) as video_gen sets them (:1308-1340): which of (1) prediction / interpolation, (2) prediction
    with the future masked and (3) unconditional generation get an FVD.  All False without `sampling.fvd`."""
    d, s = config.data, config.sampling
    if not getattr(s, "fvd", False):
        return False, False, False
    condf, futrf = int(d.num_frames_cond), int(getattr(d, "num_frames_future", 0))
    condp, futrp = float(getattr(d, "prob_mask_cond", 0.0)), float(getattr(d, "prob_mask_future", 0.0))
    sync = bool(getattr(d, "prob_mask_sync", False))
    pred10 = condf + int(s.num_frames_pred) >= 10
    interp10 = condf + int(d.num_frames) + futrf >= 10
    if condp == 0.0 and futrf == 0:                         # (1) Prediction, :1313
        return pred10, False, False
    if condp == 0.0 and futrf > 0 and futrp == 0.0:         # (1) Interpolation, :1316
        return interp10, False, False
    if condp == 0.0 and futrf > 0 and futrp > 0.0:          # (1) Interp + (2) Pred, :1319
        return interp10, pred10, False
    if condp > 0.0 and futrf == 0:                          # (1) Pred + (3) Gen, :1323
        return pred10, False, pred10
    if condp > 0.0 and futrf > 0 and futrp > 0.0 and not sync:      # (1) Interp + (2) Pred + (3) Gen, :1326
        return interp10, pred10, pred10
    if condp > 0.0 and futrf > 0 and futrp > 0.0 and sync:          # (1) Interp + (3) Gen, :1329
        return interp10, False, pred10
    # condp > 0, futrf > 0, futrp == 0: none of the reference's branches (it fails on an unbound name at :1334)
    raise ValueError("fvd_gates: prob_mask_cond > 0 with future frames needs prob_mask_future > 0 (the reference has no branch for it)")


def _ctx_of(dev, scorenet):
    if scorenet is not None:
        scorenet._bind_stream()
        return scorenet._ctx
    return _package_ctx(dev)


@torch.no_grad()
def fvd_clips(parts, channels, row_step=1, scorenet=None):
    """The detector's input, built on the device in one pass: `parts` = up to three [B, T_k*C, S, S] tensors in [0, 1], in clip order
    (cond frames, pred or real, future frames) -> [ceil(B / row_step), 3, sum T_k, 224, 224] fp32 in [-1, 1].  Replaces the torch.cat,
    the [::preds_per_test] of the real clips (`row_step`), to_i3d (:1918-1923: grey repeated to RGB, BTCHW -> BCTHW) and
    preprocess_single (models/fvd/fvd.py:160-186: bilinear resize to 224, centre crop, [0, 1] -> [-1, 1]).  Square frames only.  A part
    may be a channel slice of a larger tensor (cond_original[:, :nc*C]): it is read in place."""
    parts = list(parts)
    if not 1 <= len(parts) <= 3:
        raise ValueError(f"fvd_clips: {len(parts)} parts (1 to 3: cond, pred or real, future)")
    dev = scorenet.device if scorenet is not None else (parts[0].device if parts[0].is_cuda else torch.device("cuda", torch.cuda.current_device()))
    ts = []
    for t in parts:
        t = t.to(device=dev, dtype=torch.float32)
        if t.dim() != 4:
            raise ValueError(f"fvd_clips: a part of shape {tuple(t.shape)} is not [B, T*C, S, S]")
        if t.shape[0] and (not t[0].is_contiguous() or (t.shape[0] > 1 and t.stride(0) < t[0].numel())):
            t = t.contiguous()                                  # rows may lie apart (a channel slice), but each row's frames are dense
        ts.append(t)
    B, _, H, W = ts[0].shape
    for t in ts:
        if t.shape[0] != B or tuple(t.shape[2:]) != (H, W):
            raise ValueError(f"fvd_clips: parts {[tuple(x.shape) for x in ts]} differ in rows or frame size")
        if channels in (1, 3) and t.shape[1] % channels:
            raise ValueError(f"{t.shape[1]} channels is not a multiple of {channels}")
    if row_step < 1:
        raise ValueError(f"fvd_clips: row_step must be at least 1, got {row_step!r}")
    frames = [t.shape[1] // max(channels, 1) for t in ts]       # the library refuses channels outside {1, 3} and parts of no frames
    n = len(ts)
    out = torch.empty((-(-B // row_step), 3, sum(frames), 224, 224), dtype=torch.float32, device=dev)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    nfr = (C.c_int * n)(*frames)
    strides = (C.c_int64 * n)(*[t.stride(0) if B > 1 else t[0].numel() for t in ts])
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.mcvd_fvd_clips(_ctx_of(dev, scorenet), ptrs, nfr, strides, n, B, channels, H, W, 0, row_step,
                                           C.c_void_p(out.data_ptr())), "fvd_clips")
    return out


@torch.no_grad()
def feature_stats(feats, start=0, step=1, scorenet=None):
    """(mu [d], sigma [d, d]) of feats[start::step] as fp64 device tensors: compute_stats (models/fvd/fvd.py:275-278) --
    np.mean(axis=0) and np.cov(rowvar=False) -- on the device in fp64 (mcvd_feature_stats).  feats: [N, d] fp32 or fp64, d <= 2048; at
    least two selected rows (np.cov of one row is NaN; refused)."""
    dev = scorenet.device if scorenet is not None else (feats.device if feats.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    x = torch.as_tensor(feats)
    if x.dtype not in (torch.float32, torch.float64):
        x = x.to(torch.float64)
    x = x.to(dev)
    if x.dim() != 2:
        raise ValueError(f"feature_stats: features of shape {tuple(x.shape)} are not [N, d]")
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    N, d = x.shape
    mu = torch.empty((d,), dtype=torch.float64, device=dev)
    sigma = torch.empty((d, d), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.mcvd_feature_stats(_ctx_of(dev, scorenet), C.c_void_p(x.data_ptr()), _lib.F64 if x.dtype == torch.float64 else _lib.F32,
                                               N, d, x.stride(0), start, step, C.c_void_p(mu.data_ptr()), C.c_void_p(sigma.data_ptr())),
                   "feature_stats")
    return mu, sigma


def frechet_from_stats(mu_gen, sigma_gen, mu_real, sigma_real):
    """The host part of frechet_distance (models/fvd/fvd.py:284-287) from the two (mean, covariance) pairs, in fp64 on the CPU:
    m + tr(S_g) + tr(S_r) - 2 tr sqrtm(S_g S_r), the last as the sum of Re sqrt(lambda_i) over the eigenvalues of S_g S_r."""
    mu_g, mu_r = (torch.as_tensor(v).detach().to("cpu", torch.float64) for v in (mu_gen, mu_real))
    s_g, s_r = (torch.as_tensor(v).detach().to("cpu", torch.float64) for v in (sigma_gen, sigma_real))
    m = torch.square(mu_g - mu_r).sum()
    lam = torch.linalg.eigvals(s_g @ s_r)
    tr_sqrt = torch.sqrt(lam).real.sum()
    return float(m + torch.trace(s_g) + torch.trace(s_r) - 2.0 * tr_sqrt)


def frechet_distance(feats_fake, feats_real, start=0, step=1, scorenet=None):
    """frechet_distance(feats_fake[start::step], feats_real) of models/fvd/fvd.py:281-287: the statistics on the device
    (feature_stats), the rest on the host in fp64 (frechet_from_stats).  Usable for any features up to d = 2048."""
    mu_g, s_g = feature_stats(feats_fake, start, step, scorenet=scorenet)
    mu_r, s_r = feature_stats(feats_real, scorenet=scorenet)
    return frechet_from_stats(mu_g, s_g, mu_r, s_r)


def fvd_stuff(fake_embeddings, real_embeddings, preds_per_test=1, distance=frechet_distance):
    """(fvd, fvd_traj_mean, fvd_traj_std, fvd_traj_conf95) of :2217-2229: the distance over all rows, then over each of the
    `preds_per_test` strided subsets fake[traj::ppt] (in order -- see the module docstring), np.mean / np.std of those and
    conf95 = mean - norm.interval(0.95, loc=mean, scale=sem)[0]; -1, -1, -1 when preds_per_test == 1."""
    avg = distance(fake_embeddings, real_embeddings)
    if preds_per_test <= 1:
        return avg, -1, -1, -1
    fvds = [distance(fake_embeddings, real_embeddings, traj, preds_per_test) for traj in range(preds_per_test)]
    mean, std = float(np.mean(fvds)), float(np.std(fvds))
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.float64(np.std(fvds, ddof=1) / len(fvds) ** 0.5)
    lo = _NDTRI_Q1 * scale + mean if (scale > 0 and mean == mean) else math.nan
    return avg, mean, std, mean - float(lo)


def summarize_fvd(fake_embeddings, real_embeddings, preds_per_test=1, suffix="", distance=frechet_distance):
    """The fvd keys of the reference's summary (:2239, :2262, :2269): fvd, fvd_traj_mean, fvd_traj_std, fvd_traj_conf95 with `suffix`
    ("2", "3") after "fvd"."""
    avg, mean, std, c95 = fvd_stuff(fake_embeddings, real_embeddings, preds_per_test, distance)
    k = f"fvd{suffix}"
    return {k: avg, f"{k}_traj_mean": mean, f"{k}_traj_std": std, f"{k}_traj_conf95": c95}


class _MergedOnly:
    """Stands where VideoMetrics.merged has no LpipsNet / detector to put: the merged object summarises, it does not measure."""

    def __call__(self, *a, **kw):
        raise RuntimeError("a VideoMetrics built by merged() holds no detector: it takes no further update()")

    def __getattr__(self, name):
        raise RuntimeError("a VideoMetrics built by merged() holds no LpipsNet: it takes no further update()")


class VideoMetrics:
    """Accumulates video_gen's metric lists over batches and summarises them as NCSNRunner.video_gen does in test mode.

        vm = VideoMetrics(config, preds_per_test=ppt)
        vm.update(pred01, real01, phase=1)        # per batch, [B, T*C, H, W] in [0, 1]; phase=2 for (2) "pred_future_masked"
        vm.summary()                              # {"preds_per_test", "mse", "mse_std", "mse_conf95", "psnr...", "ssim...", "...2"}

    With `lpips=LpipsNet` it also keeps vid_lpips / vid_lpips2 (zeros under "cannot calculate") and the summary gains lpips, lpips_std,
    lpips_conf95 (and lpips2...).  Without it nothing of LPIPS is computed and the key set is the one above.

    With `fvd=detector` (and `sampling.fvd` in the config) it also keeps the FVD embeddings.  The detector is the caller's: it is called
    as the reference calls its I3D (models/fvd/fvd.py:43-48), `detector(x, rescale=False, resize=False, return_features=True) -> [b, d]`
    with x the [b, 3, T, 224, 224] fp32 device tensor, on batches of `fvd_batch` clips.  update() then needs `cond01`
    (inverse_data_transform of the cond frames: cond_original / cond_original2), and update_gen(pred_uncond01) adds phase (3).  The summary
    gains fvd, fvd_traj_mean, fvd_traj_std, fvd_traj_conf95 and the fvd2... / fvd3... groups where their gates (fvd_gates) are on;
    embeddings() returns the arrays of the reference's video_embeddings_{ckpt}.npz.  Without `fvd=` nothing changes.

    Rows are grouped in consecutive runs of `preds_per_test` (the reference's collate repeat_interleaves each clip).  When `real01` has
    fewer frames than `pred01` the phase appends 0 for every row instead (:1573-1578); after that in phase (1) the reference reports no
    summary at all, and summary() returns None.  The MNIST rule follows config.data.dataset.

    A sharded evaluation (runner.evaluate_video_gen, shard=) keeps one VideoMetrics per rank: state() is what a rank hands over and
    VideoMetrics.merged(config, states) the object of the whole run, its lists in global order.  Neither changes what update(),
    update_gen(), summary() and embeddings() do without them; an update() of zero rows (an empty shard) adds nothing."""

    def __init__(self, config, preds_per_test=1, scorenet=None, lpips=None, fvd=None, fvd_batch=10):
        self.channels = int(config.data.channels)
        self.binary = str(getattr(config.data, "dataset", "")).upper() in _MNIST
        self.preds_per_test = int(preds_per_test)
        self.scorenet = scorenet
        self.lpips = lpips
        self.vid = {1: ([], []), 2: ([], [])}
        self.vid_lpips = {1: [], 2: []}
        self.cannot = {1: False, 2: False}      # the phase appended zeros ("cannot calculate")
        self._calls = []                        # (phase, rows, cannot, embedded) per update / update_gen call: what state() cuts the lists by
        self.fvd = fvd
        self.fvd_batch = int(fvd_batch)
        if fvd is not None:
            if self.fvd_batch < 1:
                raise ValueError(f"fvd_batch must be at least 1, got {fvd_batch!r}")
            self.gates = fvd_gates(config)
            self.n_cond = int(config.data.num_frames_cond)
            self.n_future = int(getattr(config.data, "num_frames_future", 0))
            # :1615-1618: phase (2) runs
            self.second_calc = (self.n_future > 0 and float(getattr(config.data, "prob_mask_future", 0.0)) > 0.0
                                and not getattr(config.data, "prob_mask_sync", False))
            # real / fake embeddings per batch, fp64 on the device: keys 1, 2, 3 = the reference's (real|fake)_embeddings, ...2, ..._uncond
            self.emb = {k: ([], []) for k in (1, 2, 3)}
            self._last_real = None              # the real embeddings of the current batch that phase (3) reuses (:1977)

    def _detect(self, clips):
        """get_feats (models/fvd/fvd.py:41-49) on preprocessed clips: batches of fvd_batch, stacked as float64."""
        out = []
        for i in range(0, len(clips), self.fvd_batch):
            f = self.fvd(clips[i:i + self.fvd_batch], rescale=False, resize=False, return_features=True)
            out.append(torch.as_tensor(f).detach().to(device=clips.device, dtype=torch.float64).reshape(len(clips[i:i + self.fvd_batch]), -1))
        return torch.cat(out)

    def _update_fvd(self, pred01, real01, cond01, phase):
        calc1, calc2, calc3 = self.gates
        # :1925 -- (1) embeds under calc_fvd1, or under calc_fvd3 when there is no phase (2); :1956 -- (2) under calc_fvd2 or calc_fvd3
        on = (calc1 or (calc3 and not self.second_calc)) if phase == 1 else (calc2 or calc3)
        if not on:
            return
        if cond01 is None:
            raise ValueError("VideoMetrics.update: a detector is set (fvd=) and this phase's FVD gate is on: cond01 is needed")
        Cc = self.channels
        cond = cond01[:, :self.n_cond * Cc]
        futr = [cond01[:, cond01.shape[1] - self.n_future * Cc:]] if (phase == 1 and self.n_future > 0) else []
        real = self._detect(fvd_clips([cond, real01] + futr, Cc, row_step=self.preds_per_test, scorenet=self.scorenet))
        fake = self._detect(fvd_clips([cond, pred01] + futr, Cc, scorenet=self.scorenet))
        self.emb[phase][0].append(real)
        self.emb[phase][1].append(fake)
        self._last_real = real

    def update(self, pred01, real01, phase=1, cond01=None):
        if phase not in (1, 2):
            raise ValueError(f"phase must be 1 or 2, got {phase!r}")
        vid_mse, vid_ssim = self.vid[phase]
        if real01.shape[1] < pred01.shape[1]:                   # "Cannot calculate metrics" (:1573-1578, :1744-1748)
            vid_mse.extend([0] * len(pred01))
            vid_ssim.extend([0] * len(pred01))
            if self.lpips is not None:
                self.vid_lpips[phase].extend([0] * len(pred01))
            self.cannot[phase] = True
            self._calls.append((phase, len(pred01), True, False))
            return
        if len(pred01) == 0:                                    # an empty shard of a sharded evaluation: nothing to add
            self._calls.append((phase, 0, False, False))
            return
        n_emb = len(self.emb[phase][0]) if self.fvd is not None else 0
        if self.fvd is not None:                                # the whole of `real`, before it is cut to the predicted frames (:1925-1972)
            self._update_fvd(pred01, real01, cond01, phase)
        self._calls.append((phase, len(pred01), False, self.fvd is not None and len(self.emb[phase][0]) > n_emb))
        real01 = real01[:, :pred01.shape[1]]                    # frames jj < num_frames_pred only
        mse, ssim = frame_metrics(pred01, real01, self.channels, binary=self.binary, scorenet=self.scorenet)
        m, s = video_values(mse, ssim)
        vid_mse.extend(m)
        vid_ssim.extend(s)
        if self.lpips is not None:
            self.vid_lpips[phase].extend(video_lpips(frame_lpips(pred01, real01, self.channels, self.lpips)))

    def update_gen(self, pred_uncond01):
        """Phase (3), unconditional generation (:1974-1982), after the batch's update() calls: the fake clips are the unconditional
        prediction alone (no cond frames prepended); the real embeddings of the batch are those phase (2) made if it ran, else phase
        (1)'s -- reused, not recomputed."""
        if self.fvd is None:
            raise ValueError("VideoMetrics.update_gen: no detector (fvd=) was given")
        if not self.gates[2]:
            return
        if len(pred_uncond01) == 0:                             # an empty shard of a sharded evaluation
            self._calls.append((3, 0, False, False))
            return
        if self._last_real is None:
            raise ValueError("VideoMetrics.update_gen before this batch's update(): phase (3) reuses that call's real embeddings")
        self.emb[3][0].append(self._last_real)
        self.emb[3][1].append(self._detect(fvd_clips([pred_uncond01], self.channels, scorenet=self.scorenet)))
        self._calls.append((3, len(pred_uncond01), False, True))

    def state(self):
        """What a rank of a sharded evaluation hands over (picklable, host-side): per update() / update_gen() call, in call order -- that is
        per batch and phase --, {"phase", "rows", "cannot", "mse", "ssim", "lpips", "real", "fake"}: the per-video values of the call's rows
        as the lists hold them (lpips None without an LpipsNet) and the call's real and fake embeddings as fp64 host arrays (None where
        the call embedded nothing)."""
        calls, at, at_emb = [], {1: 0, 2: 0}, {1: 0, 2: 0, 3: 0}
        for phase, rows, cannot, embedded in self._calls:
            c = {"phase": phase, "rows": rows, "cannot": cannot, "mse": None, "ssim": None, "lpips": None, "real": None, "fake": None}
            if phase in (1, 2):
                a = at[phase]
                c["mse"], c["ssim"] = list(self.vid[phase][0][a:a + rows]), list(self.vid[phase][1][a:a + rows])
                if self.lpips is not None:
                    c["lpips"] = list(self.vid_lpips[phase][a:a + rows])
                at[phase] = a + rows
            if embedded:
                j = at_emb[phase]
                c["real"], c["fake"] = (self.emb[phase][w][j].detach().to("cpu", torch.float64).numpy() for w in (0, 1))
                at_emb[phase] = j + 1
            calls.append(c)
        return {"preds_per_test": self.preds_per_test, "lpips": self.lpips is not None, "fvd": self.fvd is not None, "calls": calls}

    @classmethod
    def merged(cls, config, states, scorenet=None, device=None):
        """The VideoMetrics of the whole evaluation from the state() of every rank, in rank order: the lists in global order -- batch-major,
        the ranks in order inside a batch, which is the row order of dist.shard_rows' contiguous clip shards.  The result serves summary(),
        embeddings() and state(); it holds no LpipsNet and no detector, so it takes no further update().  The embeddings go to
        `scorenet`'s device (or `device`, default the current one), where summary() forms the FVD statistics."""
        states = list(states)
        if not states:
            raise ValueError("VideoMetrics.merged: no states")
        first = states[0]
        for st in states:
            if (st["preds_per_test"], st["lpips"], st["fvd"]) != (first["preds_per_test"], first["lpips"], first["fvd"]) \
                    or [c["phase"] for c in st["calls"]] != [c["phase"] for c in first["calls"]]:
                raise ValueError("VideoMetrics.merged: the states are not those of one evaluation (settings or call sequences differ)")
        refuse = _MergedOnly()
        vm = cls(config, preds_per_test=first["preds_per_test"], scorenet=scorenet, lpips=refuse if first["lpips"] else None,
                 fvd=refuse if first["fvd"] else None)
        if first["fvd"]:
            dev = scorenet.device if scorenet is not None else (device if device is not None else torch.device("cuda", torch.cuda.current_device()))
        for j, c0 in enumerate(first["calls"]):
            phase = c0["phase"]
            for st in states:
                c = st["calls"][j]
                if phase in (1, 2):
                    vm.vid[phase][0].extend(c["mse"])
                    vm.vid[phase][1].extend(c["ssim"])
                    if first["lpips"]:
                        vm.vid_lpips[phase].extend(c["lpips"])
                    vm.cannot[phase] = vm.cannot[phase] or c["cannot"]
                embedded = c["real"] is not None
                if embedded:
                    vm.emb[phase][0].append(torch.from_numpy(np.asarray(c["real"], dtype=np.float64)).to(dev))
                    vm.emb[phase][1].append(torch.from_numpy(np.asarray(c["fake"], dtype=np.float64)).to(dev))
                vm._calls.append((phase, c["rows"], c["cannot"], embedded))
        return vm

    def _cat(self, k, which):
        return torch.cat(self.emb[k][which]) if self.emb[k][which] else None

    def embeddings(self):
        """The six arrays of the reference's video_embeddings_{ckpt}.npz (:2271-2278) as float64 numpy arrays; a group that was not
        computed is an empty list, as the reference saves it."""
        if self.fvd is None:
            raise ValueError("VideoMetrics.embeddings: no detector (fvd=) was given")
        out = {}
        for k, suffix in ((1, ""), (2, "2"), (3, "3")):
            for which, name in ((0, "real"), (1, "fake")):
                e = self._cat(k, which)
                out[f"{name}_embeddings{suffix}"] = [] if e is None else e.cpu().numpy()
        return out

    def _fvd_keys(self, k, suffix):
        dist = lambda fake, real, start=0, step=1: frechet_distance(fake, real, start, step, scorenet=self.scorenet)      # noqa: E731
        return summarize_fvd(self._cat(k, 1), self._cat(k, 0), self.preds_per_test, suffix, dist)

    def summary(self):
        """The reference's vid_metrics without ckpt (without the lpips keys unless an LpipsNet was given, without the fvd keys unless a
        detector was given and the gates are on), in the reference's key order; None where phase (1) could not calculate (video_gen
        returns None there, :1987-1989, :2192)."""
        if self.cannot[1]:
            return None
        out = {"preds_per_test": self.preds_per_test}
        out.update(summarize(*self.vid[1], self.preds_per_test))
        if self.lpips is not None:
            out.update(summarize_lpips(self.vid_lpips[1], self.preds_per_test))
        gates = self.gates if self.fvd is not None else (False, False, False)
        if gates[0]:
            out.update(self._fvd_keys(1, ""))
        if self.vid[2][0]:
            out.update(summarize(*self.vid[2], self.preds_per_test, suffix="2"))
            if self.lpips is not None:
                out.update(summarize_lpips(self.vid_lpips[2], self.preds_per_test, suffix="2"))
            if gates[1]:
                out.update(self._fvd_keys(2, "2"))
        if gates[2]:
            out.update(self._fvd_keys(3, "3"))
        return out


# ---- fast_fid: FID, precision and recall (evaluation/fid_PR.py) --------------------------------------------------------------------------

def _feature_rows(x, dev, what):
    """[N, d] fp32 / fp64 rows on `dev` with unit column stride (a column slice of a wider matrix is read in place)."""
    x = torch.as_tensor(x)
    if x.dtype not in (torch.float32, torch.float64):
        x = x.to(torch.float64)
    if x.dim() != 2:
        raise ValueError(f"{what}: features of shape {tuple(x.shape)} are not [N, d]")
    x = x.detach().to(dev)
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return x


def _feature_device(scorenet, *tensors):
    if scorenet is not None:
        return scorenet.device
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device())


def _dtype_code(x):
    return _lib.F64 if x.dtype == torch.float64 else _lib.F32


@torch.no_grad()
def knn_radii(feats, k=3, scorenet=None):
    """Squared k-nearest-neighbour radii, an fp64 [N] device tensor: radii2[i] = the (k+1)-th smallest squared distance from row i to all
    rows, itself included -- cdist(X, X).kthvalue(k + 1).values ** 2 of calculate_precision_recall_full (evaluation/fid_PR.py:251) -- in
    fp64 on the device without the N x N matrix (mcvd_knn_radii).  feats: [N, d] fp32 or fp64, d <= 2048, 1 <= k <= 7, N >= k + 1."""
    dev = _feature_device(scorenet, feats)
    x = _feature_rows(feats, dev, "knn_radii")
    N, d = x.shape
    out = torch.empty((N,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.mcvd_knn_radii(_ctx_of(dev, scorenet), C.c_void_p(x.data_ptr()), _dtype_code(x), N, d, x.stride(0), int(k),
                                           C.c_void_p(out.data_ptr())), "knn_radii")
    return out


@torch.no_grad()
def manifold_hits(query, ref, ref_radii2, scorenet=None):
    """bool [Nq] on the device: query row i lies within the radius of some ref row, dist2(query_i, ref_j) <= ref_radii2[j] --
    (dist <= NNk).any(dim=1) of fid_PR.py:256 / :258 on squared distances, in fp64, without the Nq x Nr matrix (mcvd_manifold_hits).
    The verdict of a row does not depend on the other query rows: queries handed over in several calls get the same verdicts."""
    dev = _feature_device(scorenet, query, ref)
    q, r = _feature_rows(query, dev, "manifold_hits"), _feature_rows(ref, dev, "manifold_hits")
    if q.shape[1] != r.shape[1]:
        raise ValueError(f"manifold_hits: query rows have {q.shape[1]} features, ref rows {r.shape[1]}")
    rad = torch.as_tensor(ref_radii2).detach().to(device=dev, dtype=torch.float64).contiguous()
    if rad.shape != (r.shape[0],):
        raise ValueError(f"manifold_hits: {tuple(rad.shape)} radii for {r.shape[0]} ref rows")
    out = torch.empty((q.shape[0],), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.mcvd_manifold_hits(_ctx_of(dev, scorenet), C.c_void_p(q.data_ptr()), _dtype_code(q), q.shape[0], q.stride(0),
                                               C.c_void_p(r.data_ptr()), _dtype_code(r), r.shape[0], r.stride(0), q.shape[1],
                                               C.c_void_p(rad.data_ptr()), C.c_void_p(out.data_ptr())), "manifold_hits")
    return out.bool()


@torch.no_grad()
def precision_recall(feat_r, feat_g, k=3, return_rows=False, scorenet=None):
    """(precision, recall) of calculate_precision_recall (fid_PR.py:262-269) as Python floats: precision = the share of generated rows
    inside the real manifold (the union of the balls around every real row up to its k-th neighbour), recall = the share of real rows
    inside the generated manifold; hits.sum() / N.  The reference's `save_cpu_ram` / `batch_size` choose between two ways of holding its
    distance matrices, which do not exist here.  return_rows=True: (precision, recall, precision rows [Ng] bool, recall rows [Nr] bool)."""
    dev = _feature_device(scorenet, feat_r, feat_g)
    r, g = _feature_rows(feat_r, dev, "precision_recall"), _feature_rows(feat_g, dev, "precision_recall")
    p_rows = manifold_hits(g, r, knn_radii(r, k, scorenet=scorenet), scorenet=scorenet)
    r_rows = manifold_hits(r, g, knn_radii(g, k, scorenet=scorenet), scorenet=scorenet)
    precision, recall = int(p_rows.sum()) / len(p_rows), int(r_rows.sum()) / len(r_rows)
    return (precision, recall, p_rows, r_rows) if return_rows else (precision, recall)


def fid_from_features(feat_r, feat_g, scorenet=None):
    """FID of two feature sets (the FID lines of get_fid_PR, fid_PR.py:295-298): feature_stats of each on the device, frechet_from_stats
    on the host."""
    mu_r, s_r = feature_stats(feat_r, scorenet=scorenet)
    mu_g, s_g = feature_stats(feat_g, scorenet=scorenet)
    return frechet_from_stats(mu_g, s_g, mu_r, s_r)


def fid_from_stats(stats, feats, scorenet=None):
    """FID of a feature set against stored statistics -- fast_fid's --no_pr branch (get_fid, fid_PR.py:315-321).  stats: (mu, sigma) or
    the path of an .npz with the keys `mu` and `sigma` (the reference's fid_stats_*.npz)."""
    if isinstance(stats, str):
        if not stats.endswith(".npz"):
            raise ValueError(f"fid_from_stats: {stats!r} is not an .npz path")
        with np.load(stats) as f:
            mu, sigma = f["mu"][:], f["sigma"][:]
    else:
        mu, sigma = stats
    mu_g, s_g = feature_stats(feats, scorenet=scorenet)
    return frechet_from_stats(mu_g, s_g, mu, sigma)


@torch.no_grad()
def get_activations(x, detector=None, batch_size=50):
    """Features [n, dims] of one fid_pr argument (get_activations / calculate_activations, fid_PR.py:272-279, :110-167):

      * a `.pt` / `.pth` path: torch.load of a feature tensor;
      * a tensor [n, dims]: features, returned as they are;
      * a tensor [n, C, H, W] of images in [0, 1]: `detector(batch)` on batches of `batch_size` rows (shrunk to n when larger, :133-136),
        each batch handed over on the device it is on.  A list or tuple result is indexed [0] (:155); a 4-D result whose H x W is not
        1 x 1 is averaged with adaptive_avg_pool2d (:159-160); rows are stored as fp32, as the reference's `pred_arr`."""
    if isinstance(x, str):
        if not (x.endswith(".pt") or x.endswith(".pth")):
            raise ValueError(f"fid_pr: {x!r} is not a .pt or .pth path")
        x = torch.load(x, map_location="cpu", weights_only=True)
    if not torch.is_tensor(x):
        raise TypeError(f"fid_pr: a feature tensor, an image tensor or a .pt / .pth path is needed, got {type(x).__name__}")
    if x.dim() == 2:
        return x
    if x.dim() != 4:
        raise ValueError(f"fid_pr: a tensor of shape {tuple(x.shape)} is neither features [n, dims] nor images [n, C, H, W]")
    if detector is None:
        raise ValueError("fid_pr: an image tensor needs a detector, e.g. FidInception(...).load_state_dict(weights) (the package holds no "
                         "Inception weights: they are the caller's)")
    n = len(x)
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"fid_pr: batch_size must be at least 1, got {batch_size}")
    batch_size = min(batch_size, n)
    out = []
    for i in range(0, n, batch_size):
        pred = detector(x[i:i + batch_size])
        if isinstance(pred, (list, tuple)):
            pred = pred[0]
        pred = torch.as_tensor(pred).detach()
        if pred.dim() == 4 and (pred.shape[2] != 1 or pred.shape[3] != 1):
            pred = torch.nn.functional.adaptive_avg_pool2d(pred, output_size=(1, 1))
        out.append(pred.reshape(pred.shape[0], -1).float())
    return torch.cat(out)


def fid_pr(real, fake, detector=None, k=3, batch_size=50, save_feats_path=None, scorenet=None):
    """(fid, precision, recall) of get_fid_PR (fid_PR.py:282-299).  `real` and `fake` are each a feature tensor, a `.pt` / `.pth` path of
    features or an image tensor (see get_activations; images need `detector`: FidInception with the caller's weights, or any callable).
    save_feats_path: the generated features are torch.save()d there (on the CPU), as the reference does for its feats_{ckpt}.pt."""
    feat_r = get_activations(real, detector, batch_size)
    feat_g = get_activations(fake, detector, batch_size)
    if save_feats_path is not None:
        torch.save(feat_g.detach().cpu(), save_feats_path)
    precision, recall = precision_recall(feat_r, feat_g, k, scorenet=scorenet)
    return fid_from_features(feat_r, feat_g, scorenet=scorenet), precision, recall


def _inception_a(p, cin, pf):
    return [(p + ".branch1x1", 64, cin, 1, 1), (p + ".branch5x5_1", 48, cin, 1, 1), (p + ".branch5x5_2", 64, 48, 5, 5),
            (p + ".branch3x3dbl_1", 64, cin, 1, 1), (p + ".branch3x3dbl_2", 96, 64, 3, 3), (p + ".branch3x3dbl_3", 96, 96, 3, 3),
            (p + ".branch_pool", pf, cin, 1, 1)]


def _inception_c(p, cin, c7):
    return [(p + ".branch1x1", 192, cin, 1, 1), (p + ".branch7x7_1", c7, cin, 1, 1), (p + ".branch7x7_2", c7, c7, 1, 7),
            (p + ".branch7x7_3", 192, c7, 7, 1), (p + ".branch7x7dbl_1", c7, cin, 1, 1), (p + ".branch7x7dbl_2", c7, c7, 7, 1),
            (p + ".branch7x7dbl_3", c7, c7, 1, 7), (p + ".branch7x7dbl_4", c7, c7, 7, 1), (p + ".branch7x7dbl_5", 192, c7, 1, 7),
            (p + ".branch_pool", 192, cin, 1, 1)]


def _inception_e(p, cin):
    return [(p + ".branch1x1", 320, cin, 1, 1), (p + ".branch3x3_1", 384, cin, 1, 1), (p + ".branch3x3_2a", 384, 384, 1, 3),
            (p + ".branch3x3_2b", 384, 384, 3, 1), (p + ".branch3x3dbl_1", 448, cin, 1, 1), (p + ".branch3x3dbl_2", 384, 448, 3, 3),
            (p + ".branch3x3dbl_3a", 384, 384, 1, 3), (p + ".branch3x3dbl_3b", 384, 384, 3, 1), (p + ".branch_pool", 192, cin, 1, 1)]


# The 94 BasicConv2d layers of the FID InceptionV3 in torchvision's module order: (name, Cout, Cin, kh, kw) = the shape of
# `<name>.conv.weight`; `<name>.bn.weight|bias|running_mean|running_var` are [Cout].  Strides and paddings live in kernels/inception.cpp.
FID_INCEPTION_CONVS = tuple(
    [("Conv2d_1a_3x3", 32, 3, 3, 3), ("Conv2d_2a_3x3", 32, 32, 3, 3), ("Conv2d_2b_3x3", 64, 32, 3, 3), ("Conv2d_3b_1x1", 80, 64, 1, 1),
     ("Conv2d_4a_3x3", 192, 80, 3, 3)]
    + _inception_a("Mixed_5b", 192, 32) + _inception_a("Mixed_5c", 256, 64) + _inception_a("Mixed_5d", 288, 64)
    + [("Mixed_6a.branch3x3", 384, 288, 3, 3), ("Mixed_6a.branch3x3dbl_1", 64, 288, 1, 1), ("Mixed_6a.branch3x3dbl_2", 96, 64, 3, 3),
       ("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 3)]
    + _inception_c("Mixed_6b", 768, 128) + _inception_c("Mixed_6c", 768, 160) + _inception_c("Mixed_6d", 768, 160)
    + _inception_c("Mixed_6e", 768, 192)
    + [("Mixed_7a.branch3x3_1", 192, 768, 1, 1), ("Mixed_7a.branch3x3_2", 320, 192, 3, 3), ("Mixed_7a.branch7x7x3_1", 192, 768, 1, 1),
       ("Mixed_7a.branch7x7x3_2", 192, 192, 1, 7), ("Mixed_7a.branch7x7x3_3", 192, 192, 7, 1), ("Mixed_7a.branch7x7x3_4", 192, 192, 3, 3)]
    + _inception_e("Mixed_7b", 1280) + _inception_e("Mixed_7c", 2048))
_FID_BN = ("weight", "bias", "running_mean", "running_var")
# every tensor FidInception.load_state_dict requires -> its shape, in the state dict's own order
FID_INCEPTION_PARAMS = {}
for _n, _co, _ci, _kh, _kw in FID_INCEPTION_CONVS:
    FID_INCEPTION_PARAMS[f"{_n}.conv.weight"] = (_co, _ci, _kh, _kw)
    for _k in _FID_BN:
        FID_INCEPTION_PARAMS[f"{_n}.bn.{_k}"] = (_co,)
del _n, _co, _ci, _kh, _kw, _k
_FID_BLOCK_SHAPES = ((64, 73, 73), (192, 35, 35), (768, 17, 17), (2048, 1, 1))


class FidInception(_DeviceNet):
    """The reference's evaluation.inception.InceptionV3(output_blocks, resize_input, normalize_input) -- the FID variant
    (use_fid_inception=True), eval mode, no gradients -- on the device, as a `detector=` for fid_pr, fast_fid and NearestNeighbors:

        det = FidInception(scorenet=hipnet).load_state_dict("pt_inception-2015-12-05-6726825d.pth")      # or FidInception(device="cuda:0")
        feats = det(images01)[0]                                # [n, 2048, 1, 1]; a list in ascending block order, as InceptionV3.forward

    output_blocks: any of 0 (first max pool, 64 x 73 x 73), 1 (second max pool, 192 x 35 x 35), 2 (Mixed_6e, 768 x 17 x 17), 3 (the final
    average pool, 2048 x 1 x 1); the net runs up to the highest one.  The weights are the caller's: load_state_dict takes the reference's
    file (a path or its dict) by its own key names and the package holds and downloads none.  Runs on the scorenet's context and stream
    when given one, else on this module's own context (as LpipsNet).  Missing weights are an error at the first use (MCVD_ESTATE names
    the tensor).  There is no CPU fallback."""

    _KIND = "inception"

    def __init__(self, output_blocks=(3,), resize_input=True, normalize_input=True, device=None, scorenet=None):
        self._require_gpu()      # the order of the errors: no GPU, then bad arguments, before anything is created
        blocks = sorted(set(int(b) for b in output_blocks))
        if not blocks or blocks[0] < 0 or blocks[-1] > 3:
            raise ValueError(f"FidInception: output_blocks {tuple(output_blocks)} must be a non-empty subset of 0..3")
        self.output_blocks, self.resize_input, self.normalize_input = blocks, bool(resize_input), bool(normalize_input)
        super().__init__(device, scorenet)

    def load_state_dict(self, sd_or_path):
        """The reference's pt_inception-2015-12-05-6726825d.pth (path or dict): `X.conv.weight`, `X.bn.weight|bias|running_mean|running_var`.
        `fc.*`, `AuxLogits.*` and `*.num_batches_tracked` are ignored; any other unknown key and any wrong shape is a ValueError.  A
        partial dict is accepted (what is still missing is named at the first use)."""
        sd = sd_or_path
        if not isinstance(sd, dict):
            sd = torch.load(sd, map_location="cpu", weights_only=True)
        for name, t in sd.items():
            if name.startswith("fc.") or name.startswith("AuxLogits.") or name.endswith(".num_batches_tracked"):
                continue
            want = FID_INCEPTION_PARAMS.get(name)
            if want is None:
                raise ValueError(f"FidInception.load_state_dict: unknown key {name!r}")
            if tuple(t.shape) != want:
                raise ValueError(f"FidInception.load_state_dict: {name} has shape {tuple(t.shape)}, expected {want}")
            self._set(name, t)
        return self

    @torch.no_grad()
    def __call__(self, images):
        """images [n, 3, H, W] in [0, 1] -> the requested blocks' outputs, a list of fp32 device tensors in ascending block order."""
        if not torch.is_tensor(images) or images.dim() != 4:
            raise ValueError("FidInception: images must be a tensor [n, 3, H, W]")
        n, ch, H, W = images.shape
        if ch != 3:
            raise ValueError(f"FidInception: {ch}-channel images (Conv2d_1a_3x3 takes 3 channels)")
        if n < 1:
            raise ValueError("FidInception: no images")
        if not self.resize_input and (H, W) != (299, 299):
            raise ValueError(f"FidInception: resize_input=False needs 299 x 299 images, got {H} x {W}")
        x = images.detach().to(device=self.device, dtype=torch.float32).contiguous()
        self.finalize()
        outs = [None] * 4
        mask = 0
        for b in self.output_blocks:
            outs[b] = torch.empty((n,) + _FID_BLOCK_SHAPES[b], dtype=torch.float32, device=self.device)
            mask |= 1 << b
        with torch.cuda.device(self.device):
            self._ctx()
            ptrs = [C.c_void_p(o.data_ptr()) if o is not None else None for o in outs]
            _lib.check(_lib.lib.mcvd_inception_forward(self._net, C.c_void_p(x.data_ptr()), n, H, W, int(self.resize_input),
                                                       int(self.normalize_input), mask, *ptrs), "inception_forward")
        return [outs[b] for b in self.output_blocks]


# ---- nearest neighbours of samples in a data set (evaluation/nearest_neighbor.py) -----------------------------------------------------------

@torch.no_grad()
def knn_search(query, ref, k=10, query2=None, index_base=0, state=None, scorenet=None):
    """(dist2 [Nq, k] fp64, index [Nq, k] int64) on the device: the k ref rows nearest to every query row -- torch.cdist, torch.min and
    topk(-d, k) of get_nearest_neighbors (nearest_neighbor.py:102-109) in fp64 without the Nq x Nr matrices (mcvd_knn_search).  With
    `query2`, a second view of the same queries, a pair's distance is the smaller of the two.  Rows are ascending by (squared distance,
    index), equal distances lower index first; index = index_base + the ref row; with fewer than k candidates the tail holds +inf / -1.
    state=(dist2, index) of an earlier call continues that search: pieces of a data set in any split give the result of one call, bit
    for bit.  query / query2 / ref: [N, d] fp32 or fp64, d <= 2048, 1 <= k <= 16."""
    dev = _feature_device(scorenet, query, ref)
    q, r = _feature_rows(query, dev, "knn_search"), _feature_rows(ref, dev, "knn_search")
    q2 = None if query2 is None else _feature_rows(query2, dev, "knn_search")
    if q.shape[1] != r.shape[1]:
        raise ValueError(f"knn_search: query rows have {q.shape[1]} features, ref rows {r.shape[1]}")
    if q2 is not None and q2.shape != q.shape:
        raise ValueError(f"knn_search: the second view is {tuple(q2.shape)}, the first {tuple(q.shape)}")
    k = int(k)
    Nq = q.shape[0]
    if state is None:
        dist2 = torch.empty((Nq, max(k, 0)), dtype=torch.float64, device=dev)
        index = torch.empty((Nq, max(k, 0)), dtype=torch.int64, device=dev)
    else:
        dist2, index = (torch.as_tensor(t).detach().to(device=dev, dtype=dt).contiguous().clone()
                        for t, dt in zip(state, (torch.float64, torch.int64)))
        if tuple(dist2.shape) != (Nq, k) or tuple(index.shape) != (Nq, k):
            raise ValueError(f"knn_search: state of shapes {tuple(dist2.shape)}, {tuple(index.shape)} for {Nq} queries and k = {k}")
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.mcvd_knn_search(_ctx_of(dev, scorenet), P(q), _dtype_code(q), q.stride(0), P(q2), _dtype_code(q2) if q2 is not None else 0,
                                            q2.stride(0) if q2 is not None else 0, Nq, P(r), _dtype_code(r), r.stride(0), r.shape[0], q.shape[1], k,
                                            int(index_base), 0 if state is None else 1, P(dist2), P(index)), "knn_search")
    return dist2, index


@torch.no_grad()
def hflip_u8(images01, scorenet=None):
    """The mirrored view of get_nearest_neighbors, to_tensor(flipper(to_pil(img))) (nearest_neighbor.py:81-83, :95), on the device
    (mcvd_hflip_u8): x.mul(255).byte(), mirrored along W, / 255.  images01: [n, C, H, W] in [0, 1] -> fp32 [n, C, H, W]."""
    dev = _feature_device(scorenet, images01)
    x = torch.as_tensor(images01).detach().to(device=dev, dtype=torch.float32).contiguous()
    if x.dim() != 4:
        raise ValueError(f"hflip_u8: images of shape {tuple(x.shape)} are not [n, C, H, W]")
    out = torch.empty_like(x)
    n, Cc, H, W = x.shape
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.mcvd_hflip_u8(_ctx_of(dev, scorenet), C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), n, Cc, H, W), "hflip_u8")
    return out


@torch.no_grad()
def nn_collect(held, held_index, new_index, piece, index_base, scorenet=None):
    """The images of the list slots after a knn_search over one piece (mcvd_nn_collect): [Nq, k, C, H, W], a slot whose index lies in
    `piece` ([n, C, H, W], first row = index_base) copied from it, any other from the slot of `held` ([Nq, k, C, H, W], listed by
    held_index) with the same index, zeros for -1.  held = held_index = None: nothing is held yet."""
    dev = new_index.device
    Nq, k = new_index.shape
    n, Cc, H, W = piece.shape
    out = torch.empty((Nq, k, Cc, H, W), dtype=torch.float32, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.mcvd_nn_collect(_ctx_of(dev, scorenet), P(held), P(held_index), P(new_index), P(piece), n, int(index_base), Nq, k, Cc, H, W,
                                            P(out)), "nn_collect")
    return out


def detector_features(detector, images):
    """get_activations of nearest_neighbor.py:45-55: `detector(images)[0]` on the whole batch in ONE call (not in batches of 50 as
    fid_PR.py's), adaptive_avg_pool2d when the maps are not 1 x 1, reshape(n, -1); rows as fp32, as the reference's."""
    pred = detector(images)
    if isinstance(pred, (list, tuple)):
        pred = pred[0]
    pred = torch.as_tensor(pred).detach()
    if pred.dim() == 4 and (pred.shape[2] != 1 or pred.shape[3] != 1):
        pred = torch.nn.functional.adaptive_avg_pool2d(pred, output_size=(1, 1))
    return pred.reshape(pred.shape[0], -1).float()


class NearestNeighbors:
    """get_nearest_neighbors (evaluation/nearest_neighbor.py:70-114) with the data set handed over in pieces: for each of the first
    `n_samples` samples the `k` data images nearest in the detector's feature space, the distance being the smaller of the distances
    from the sample and from its mirrored copy.  Neither the data images, nor their features, nor an n x N matrix are kept: after every
    update() the state is k distances, k indices and k images per sample, all on the device.

    samples: a tensor [n, C, H, W] in [0, 1] or the path of a .pt that holds one (fast_fid's samples_{ckpt}.pt); `[:n_samples]` is applied
    as the reference does.  detector: the reference's InceptionV3([block]) is FidInception((block,)) with the caller's weights; any
    callable will do.  It is called on the whole batch.  flip=False searches with the unmirrored view alone.  Ties in distance go to the lower data index (topk leaves them open)."""

    def __init__(self, samples, detector, k=10, n_samples=10, flip=True, scorenet=None):
        if isinstance(samples, str):
            if not (samples.endswith(".pt") or samples.endswith(".pth")):
                raise ValueError(f"NearestNeighbors: {samples!r} is not a .pt or .pth path")
            samples = torch.load(samples, map_location="cpu", weights_only=True)
        if not torch.is_tensor(samples) or samples.dim() != 4:
            raise ValueError("NearestNeighbors: samples must be an image tensor [n, C, H, W] or the .pt path of one, got "
                             + (str(tuple(samples.shape)) if torch.is_tensor(samples) else type(samples).__name__))
        if detector is None:
            raise ValueError("NearestNeighbors: a detector is needed, e.g. FidInception(...).load_state_dict(weights) (the package holds no "
                             "Inception weights: they are the caller's)")
        k, n_samples = int(k), int(n_samples)
        if not 1 <= k <= 16:
            raise ValueError(f"NearestNeighbors: k = {k} is outside 1..16")
        if n_samples < 1 or len(samples) < 1:
            raise ValueError(f"NearestNeighbors: no samples (n_samples = {n_samples}, {len(samples)} rows)")
        self.k, self.detector, self.scorenet = k, detector, scorenet
        self.device = _feature_device(scorenet, samples)
        self.samples = samples[:n_samples].detach().to(device=self.device, dtype=torch.float32).contiguous()
        self.flipped = hflip_u8(self.samples, scorenet=scorenet) if flip else None
        self.feats = detector_features(detector, self.samples)
        self.feats2 = detector_features(detector, self.flipped) if flip else None
        self.seen = 0
        self.state = None               # (dist2, index)
        self.held = None                # [n, k, C, H, W]

    @torch.no_grad()
    def update(self, images, feats=None):
        """One piece of the data set: images [m, C, H, W] in [0, 1], in data-set order; feats [m, d], or None for detector(images)."""
        x = torch.as_tensor(images).detach().to(device=self.device, dtype=torch.float32).contiguous()
        if x.dim() != 4 or tuple(x.shape[1:]) != tuple(self.samples.shape[1:]):
            raise ValueError(f"NearestNeighbors.update: images of shape {tuple(x.shape)} beside samples of shape {tuple(self.samples.shape)}")
        f = detector_features(self.detector, x) if feats is None else torch.as_tensor(feats)
        if f.dim() != 2 or len(f) != len(x):
            raise ValueError(f"NearestNeighbors.update: features of shape {tuple(f.shape)} for {len(x)} images")
        if len(x) == 0:
            return
        old = self.state
        self.state = knn_search(self.feats, f, self.k, query2=self.feats2, index_base=self.seen, state=old, scorenet=self.scorenet)
        self.held = nn_collect(self.held, None if old is None else old[1], self.state[1], x, self.seen, scorenet=self.scorenet)
        self.seen += len(x)

    def result(self):
        """indices [n, k] int64, distances [n, k] fp64 (Euclidean, ascending), neighbors [n, k, C, H, W] and plot_data [n (k + 1), C, H, W]
        -- sample i followed by its k neighbours, what the reference hands to save_image(..., nrow=k + 1)."""
        if self.seen < self.k:
            raise RuntimeError(f"NearestNeighbors: k = {self.k} neighbours of {self.seen} data rows (the reference's topk raises there)")
        dist2, index = self.state
        plot = torch.cat([self.samples[:, None], self.held], 1).reshape(-1, *self.samples.shape[1:])
        return {"indices": index, "distances": dist2.sqrt(), "neighbors": self.held, "plot_data": plot}
