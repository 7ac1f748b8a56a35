"""The numbers video_gen's test mode reports per phase: MSE, PSNR, SSIM and LPIPS (runners/ncsn_runner.py:1580-1609, :1749-1778,
:2195-2255), with the per-frame work on the device (mcvd_frame_metrics, kernels/metrics.cpp; mcvd_lpips_frames, kernels/lpips.cpp) and the
per-video / summary arithmetic on the host in the reference's dtypes and order.

LPIPS (v0.1, AlexNet, "net-lin") is computed when the caller hands VideoMetrics an LpipsNet that holds the weights: the backbone is
torchvision's AlexNet `features` state dict and the five lin layers are the reference's models/weights/v0.1/alex.pth, both supplied by the
caller as a MCVD checkpoint is -- the package ships no weights, downloads none and has no default.  The ScalingLayer's six constants are
part of the architecture (models/networks_basic.py:93-94) and are set at construction.  FVD is not computed: its I3D network is a
TorchScript file, not an architecture one can restate.

Deliberate divergences from the reference:
  * frames of 2 or 4 channels (torchvision's LA / RGBA images) are refused with ValueError: no MCVD dataset has them;
  * :1742-1747: phase (2) tests phase (1)'s `real` / `pred` shapes and, when it cannot compute, appends its zeros to phase (1)'s lists.
    Here phase (2) tests its own frames and appends to its own lists.
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


class LpipsNet:
    """The reference's eval_models.PerceptualLoss(model='net-lin', net='alex') (version 0.1, eval mode) on the device.

        net = LpipsNet(scorenet=hipnet)                       # or LpipsNet(device="cuda:0")
        net.load_backbone(torchvision_alexnet_state_dict)     # keys features.N.weight / bias; classifier keys are ignored
        net.load_linear("weights/v0.1/alex.pth")              # the reference's lin layers (path or state dict)
        # or net.load_state_dict(pnetlin.state_dict()) for a whole PNetLin dict

    Runs on the scorenet's context and stream when given one, else on this module's own context (as frame_metrics).  Missing weights are
    an error at the first use (MCVD_ESTATE names the tensor)."""

    def __init__(self, device=None, scorenet=None):
        if not torch.cuda.is_available():
            raise RuntimeError("LpipsNet needs a ROCm GPU (MI355X); there is no CPU fallback")
        self.scorenet = scorenet
        if scorenet is not None:
            self.device = scorenet.device
        else:
            dev = torch.device(device if device is not None else "cuda")
            self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self._net = C.c_void_p()
        self._final = False
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib.mcvd_lpips_create(self._ctx(), C.byref(self._net)), "lpips_create")
        # ScalingLayer (models/networks_basic.py:93-94): constants of the architecture, not learned weights
        self._set("scaling_layer.shift", torch.tensor([-.030, -.088, -.188]))
        self._set("scaling_layer.scale", torch.tensor([.458, .448, .450]))

    def _ctx(self):
        if self.scorenet is not None:
            self.scorenet._bind_stream()
            return self.scorenet._ctx
        return _package_ctx(self.device)

    def _set(self, name, t):
        t = t.detach().to(device="cpu", dtype=torch.float32).contiguous()
        shape = (C.c_int64 * t.dim())(*t.shape)
        _lib.check(_lib.lib.mcvd_lpips_set_param(self._net, name.encode(), C.c_void_p(t.data_ptr()), shape, t.dim(), 0), f"lpips_set_param({name})")
        self._final = False

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

    def finalize(self):
        if not self._final:
            with torch.cuda.device(self.device):
                self._ctx()
                _lib.check(_lib.lib.mcvd_lpips_finalize(self._net), "lpips_finalize")
            self._final = True
        return self

    def __del__(self):
        try:
            if getattr(self, "_net", None):
                _lib.lib.mcvd_lpips_destroy(self._net)
                self._net = None
        except Exception:
            pass


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


class VideoMetrics:
    """Accumulates video_gen's metric lists over batches and summarises them as NCSNRunner.video_gen does in test mode.

        vm = VideoMetrics(config, preds_per_test=ppt)
        vm.update(pred01, real01, phase=1)        # per batch, [B, T*C, H, W] in [0, 1]; phase=2 for (2) "pred_future_masked"
        vm.summary()                              # {"preds_per_test", "mse", "mse_std", "mse_conf95", "psnr...", "ssim...", "...2"}

    With `lpips=LpipsNet` it also keeps vid_lpips / vid_lpips2 (zeros under "cannot calculate") and the summary gains lpips, lpips_std,
    lpips_conf95 (and lpips2...).  Without it nothing of LPIPS is computed and the key set is the one above.

    Rows are grouped in consecutive runs of `preds_per_test` (the reference's collate repeat_interleaves each clip).  When `real01` has
    fewer frames than `pred01` the phase appends 0 for every row instead (:1573-1578); after that in phase (1) the reference reports no
    summary at all, and summary() returns None.  The MNIST rule follows config.data.dataset."""

    def __init__(self, config, preds_per_test=1, scorenet=None, lpips=None):
        self.channels = int(config.data.channels)
        self.binary = str(getattr(config.data, "dataset", "")).upper() in _MNIST
        self.preds_per_test = int(preds_per_test)
        self.scorenet = scorenet
        self.lpips = lpips
        self.vid = {1: ([], []), 2: ([], [])}
        self.vid_lpips = {1: [], 2: []}
        self.cannot = {1: False, 2: False}      # the phase appended zeros ("cannot calculate")

    def update(self, pred01, real01, phase=1):
        if phase not in (1, 2):
            raise ValueError(f"phase must be 1 or 2, got {phase!r}")
        vid_mse, vid_ssim = self.vid[phase]
        if real01.shape[1] < pred01.shape[1]:                   # "Cannot calculate metrics" (:1573-1578, :1744-1748)
            vid_mse.extend([0] * len(pred01))
            vid_ssim.extend([0] * len(pred01))
            if self.lpips is not None:
                self.vid_lpips[phase].extend([0] * len(pred01))
            self.cannot[phase] = True
            return
        real01 = real01[:, :pred01.shape[1]]                    # frames jj < num_frames_pred only
        mse, ssim = frame_metrics(pred01, real01, self.channels, binary=self.binary, scorenet=self.scorenet)
        m, s = video_values(mse, ssim)
        vid_mse.extend(m)
        vid_ssim.extend(s)
        if self.lpips is not None:
            self.vid_lpips[phase].extend(video_lpips(frame_lpips(pred01, real01, self.channels, self.lpips)))

    def summary(self):
        """The reference's vid_metrics without ckpt (and without the lpips keys unless an LpipsNet was given); None where phase (1) could not calculate (video_gen returns None there,
        :1987-1989, :2192)."""
        if self.cannot[1]:
            return None
        out = {"preds_per_test": self.preds_per_test}
        out.update(summarize(*self.vid[1], self.preds_per_test))
        if self.lpips is not None:
            out.update(summarize_lpips(self.vid_lpips[1], self.preds_per_test))
        if self.vid[2][0]:
            out.update(summarize(*self.vid[2], self.preds_per_test, suffix="2"))
            if self.lpips is not None:
                out.update(summarize_lpips(self.vid_lpips[2], self.preds_per_test, suffix="2"))
        return out
