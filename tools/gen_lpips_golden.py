"""Golden vectors of LPIPS as the REAL reference computes it -- build container only (needs the reference checkout, scipy and Pillow).

    PYTHONDONTWRITEBYTECODE=1 python -m tools.gen_lpips_golden [direct smmnist cityscapes]

Modelled on tools/gen_video_metrics_golden.py.  The real `eval_models.PerceptualLoss(model='net-lin', net='alex')` is constructed
through the real `DistModel`, which loads the real `models/weights/v0.1/alex.pth` itself (models/dist_model.py:66-72).  Replaced from the
outside, nothing else:
  * `pretrained_networks.tv.alexnet` -> an object whose `.features` is torchvision's AlexNet feature stack restated (thirteen layers) with
    SEEDED weights (tests/lpips_ref.py: make_backbone, one generator per tensor keyed by name; randn * sqrt(2 / fan_in), biases
    0.1 * randn).  torchvision is not installed here, and the pretrained weights could not be fetched anyway; whether the computation is
    right does not depend on which backbone weights are loaded.  The backbone (9.9 MB) is not stored: the fixture keeps the seed, the
    recipe's name and per tensor its fp64 sum and 64 probed values;
  * `Transforms.Resize / ToTensor / Normalize / Compose` -> restatements that call the REAL Pillow `resize(..., BILINEAR)`;
    `Transforms.ToPILImage` as tools/gen_video_metrics_golden.py restates it.
Each fixture also stores the reference's own fp32-against-fp64 deviation: steps 4-5 are evaluated a second time in fp64 by
tests/lpips_ref.py, and `ref_rel_dev` = max over frames of |fp32 - fp64| / fp64 (the identical pair must be exactly 0 on both sides).
Nothing is written when `ref_rel_dev` exceeds 1e-4 (a sanity cap, not a tolerance: it separates fp32 rounding from a wrong restatement),
when the restated integer resize differs from Pillow's planes, when a tap of a fixture image has fewer than a fifth of its values
non-zero, or when a stored frame distance is not > 0 (except the deliberately identical pair).

tests/golden/lpips_direct.pt (frames handed straight to steps 1-5):
    seed, recipe, probes {name: (fp64 sum, 64 values)}, lins [5 x [C]], shift, scale, state_dict_names (of the real PNetLin),
    cases [{name, channels, B, T}], frames_<name> [2 (pred, real), B, T*C, H, W], resized_<name> uint8 [2, B, T, C, 128, 128] from Pillow,
    value_<name> fp32 [B, T], per_tap_<name> fp32 [B, T, 5], value64_<name> / per_tap64_<name> (the fp64 restatement), ref_rel_dev,
    tap_images (case, which, b, t) x 2 and tap<k>_real fp32 [2, C_k, H_k, W_k]: the real net's five tap tensors of those two images
tests/golden/lpips_runner_<case>.pt (the real video_gen run of video_metrics_<case>.pt's case, the same frames):
    frame values per phase and batch, vid_lpips / vid_lpips2, metric_arrays, vid_metrics (with its lpips keys), value64, ref_rel_dev
"""
import contextlib
import io
import os
import sys
import types
from unittest import mock

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from oracle.gen_runner_golden import import_real_runner  # noqa: E402
from tests import lpips_ref  # noqa: E402
from tests.golden_io import load_golden  # noqa: E402
from tools import gen_video_metrics_golden as gvm  # noqa: E402
from tools.gen_video_tasks_golden import OUT, _save  # noqa: E402

SEED = 7
CAP = 1e-4


def alexnet_features(seed):
    """torchvision.models.alexnet().features restated, with the seeded weights."""
    nn = torch.nn
    f = nn.Sequential(nn.Conv2d(3, 64, 11, 4, 2), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2), nn.Conv2d(64, 192, 5, padding=2), nn.ReLU(inplace=True),
                      nn.MaxPool2d(3, 2), nn.Conv2d(192, 384, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(384, 256, 3, padding=1),
                      nn.ReLU(inplace=True), nn.Conv2d(256, 256, 3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2))
    f.load_state_dict({k[len("features."):]: v for k, v in lpips_ref.make_backbone(seed).items()})
    return f


RESIZED = []      # the planes the real Pillow returned, in call order


class _Resize:
    def __init__(self, size):
        self.size = size

    def __call__(self, img):
        out = img.resize(self.size[::-1], Image.BILINEAR)
        RESIZED.append(np.asarray(out).copy())
        return out


class _ToTensor:
    def __call__(self, pic):
        a = np.asarray(pic)
        return torch.from_numpy(a.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


class _Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, t):
        mean, std = torch.as_tensor(self.mean, dtype=t.dtype), torch.as_tensor(self.std, dtype=t.dtype)
        return t.clone().sub_(mean[:, None, None]).div_(std[:, None, None])


class _Compose:
    def __init__(self, ts):
        self.ts = ts

    def __call__(self, x):
        for t in self.ts:
            x = t(x)
        return x


def real_perceptual(R):
    """The real PerceptualLoss over the seeded backbone; hooks record per-tap values and tap tensors of every forward."""
    import models.pretrained_networks as pn
    fake = lambda pretrained=True: types.SimpleNamespace(features=alexnet_features(SEED))      # noqa: E731
    with mock.patch.object(pn.tv, "alexnet", fake), contextlib.redirect_stdout(io.StringIO()):
        model = R.eval_models.PerceptualLoss(model='net-lin', net='alex', device=torch.device("cpu"))
    net = model.model.net
    assert not net.training and net.version == '0.1' and net.lpips and not net.spatial
    rec = dict(per_tap=[], taps=[], values=[])
    for k in range(5):
        getattr(net, f"lin{k}").model.register_forward_hook(lambda m, i, o, k=k: rec["per_tap"].append((k, o.mean([2, 3]).reshape(-1).clone())))
        getattr(net.net, f"slice{k + 1}").register_forward_hook(lambda m, i, o, k=k: rec["taps"].append((k, o.clone())))
    real_forward = model.forward

    def forward(a, b, *args, **kw):
        out = real_forward(a, b, *args, **kw)
        rec["values"].append(out.detach().reshape(-1).clone())
        return out
    model.forward = forward
    return model, net, rec


def net_constants(net):
    lins = [getattr(net, f"lin{k}").model[1].weight.detach().reshape(-1).clone() for k in range(5)]
    return lins, net.scaling_layer.shift.reshape(-1).clone(), net.scaling_layer.scale.reshape(-1).clone()


def check_and_dev(v32, v64, what):
    """-> max relative deviation; zeros must be zero on both sides; refuses above the cap."""
    v32, v64 = v32.double().reshape(-1), v64.reshape(-1)
    zero = v64 == 0
    assert torch.equal(v32[zero], v64[zero]), f"{what}: an exactly-zero distance differs"
    dev = ((v32[~zero] - v64[~zero]).abs() / v64[~zero]).max().item() if (~zero).any() else 0.0
    assert dev <= CAP, f"{what}: the fp64 restatement is {dev:.3e} away from the real PNetLin: not the same function"
    return dev


def direct_cases():
    g = torch.Generator().manual_seed(SEED)

    def noisy(B, TC, S):
        real = torch.rand(B, TC, S, S, generator=g)
        return (real + 0.2 * torch.randn(B, TC, S, S, generator=g)).clamp(0, 1), real
    cases = []
    p, r = noisy(2, 2, 64)
    cases.append(dict(name="c1_64", channels=1, pred=p, real=r))
    p, r = noisy(1, 6, 64)
    cases.append(dict(name="c3_64", channels=3, pred=p, real=r))
    # 128 x 128 (resize skipped), structured: frame 0 two constants, frame 1 a step edge against the same edge moved by 9 pixels
    p, r = torch.zeros(1, 6, 128, 128), torch.zeros(1, 6, 128, 128)
    p[:, 0:3], r[:, 0:3] = 0.3, 0.62
    p[:, 3:6, :, 64:], r[:, 3:6, :, 73:] = 0.9, 0.9
    p[:, 3:6, :, :64], r[:, 3:6, :, :73] = 0.1, 0.1
    cases.append(dict(name="c3_128_structured", channels=3, pred=p, real=r))
    # 32 x 32 (the tiny configs): frame 0 random, frame 1 an identical pair
    p, r = noisy(1, 6, 32)
    p[:, 3:6] = r[:, 3:6]
    cases.append(dict(name="c3_32_identical", channels=3, pred=p, real=r, identical=[(0, 1)]))
    p, r = noisy(1, 3, 256)
    cases.append(dict(name="c3_256", channels=3, pred=p, real=r))
    return cases


def gen_direct():
    R = import_real_runner()
    model, net, rec = real_perceptual(R)
    lins, shift, scale = net_constants(net)
    backbone = lpips_ref.make_backbone(SEED)
    T2 = _Compose([_Resize((128, 128)), _ToTensor(), _Normalize((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))])
    topil = gvm._ToPILImage()
    out = dict(seed=SEED, recipe=lpips_ref.RECIPE, probes=lpips_ref.backbone_probe(backbone), lins=lins, shift=shift, scale=scale,
               state_dict_names=list(net.state_dict().keys()), cases=[], tap_images=[("c3_64", 0, 0, 0), ("c1_64", 1, 1, 1)])
    devs, tap_store = [], {}
    for c in direct_cases():
        name, Cc, pred, real = c["name"], c["channels"], c["pred"], c["real"]
        B, T = pred.shape[0], pred.shape[1] // Cc
        del RESIZED[:], rec["per_tap"][:], rec["taps"][:], rec["values"][:]
        with torch.no_grad():
            for b in range(B):
                for t in range(T):
                    pp = topil(pred[b, Cc * t:Cc * t + Cc]).convert("RGB")
                    rp = topil(real[b, Cc * t:Cc * t + Cc]).convert("RGB")
                    model.forward(T2(rp).unsqueeze(0), T2(pp).unsqueeze(0))       # :1603-1605: pred resized first, model_lpips.forward(real, pred)
        # PerceptualLoss.forward(pred=a, target=b) calls model.forward(target, pred): in0 = pred image, in1 = real image
        planes = torch.from_numpy(np.stack(RESIZED)).reshape(B, T, 2, 128, 128, 3)       # per frame: real resized first here, then pred
        planes = planes.permute(2, 0, 1, 5, 3, 4)[[1, 0]][:, :, :, :Cc].contiguous()       # -> [2 (pred, real), B, T, C, 128, 128]
        value = torch.cat(rec["values"]).reshape(B, T)
        per_tap = torch.stack([torch.cat([v for k, v in rec["per_tap"] if k == kk]) for kk in range(5)], -1).reshape(B, T, 5)
        v64, pt64, planes_ref = lpips_ref.frame_lpips64(pred, real, Cc, backbone, lins, shift, scale)
        assert torch.equal(planes_ref, planes), f"{name}: the restated integer resize differs from Pillow {Image.__version__}"
        devs.append(check_and_dev(value, v64, name))
        check_and_dev(per_tap, pt64, name + " per tap")
        ident = {(b, t) for b, t in c.get("identical", [])}
        for b in range(B):
            for t in range(T):
                assert (value[b, t] == 0) == ((b, t) in ident), (name, b, t, value[b, t])
        # degenerate taps: every tap of every image keeps at least a fifth of its values non-zero
        for which, x in ((0, planes[0]), (1, planes[1])):
            for k, tp in enumerate(lpips_ref.taps(lpips_ref.net_input(x.reshape(B * T, Cc, 128, 128)), backbone, shift, scale)):
                frac = (tp != 0).double().mean((1, 2, 3)).min().item()
                assert frac >= 0.2, f"{name}: tap {k + 1} of image set {which} has only {frac:.2f} non-zero"
        # the real net's tap tensors: forwards in frame order, in0 = pred image then in1 = real image per forward
        for ti, (cn, which, b, t) in enumerate(out["tap_images"]):
            if cn == name:
                for k in range(5):
                    seq = [o for kk, o in rec["taps"] if kk == k]
                    tap_store.setdefault(k, {})[ti] = seq[2 * (b * T + t) + which][0]
        out["cases"].append(dict(name=name, channels=Cc, B=B, T=T))
        out[f"frames_{name}"] = torch.stack([pred, real])
        out[f"resized_{name}"] = planes
        out[f"value_{name}"], out[f"per_tap_{name}"], out[f"value64_{name}"], out[f"per_tap64_{name}"] = value, per_tap, v64, pt64
    for k in range(5):
        out[f"tap{k + 1}_real"] = torch.stack([tap_store[k][0], tap_store[k][1]])
    out["ref_rel_dev"] = max(devs)
    out["pillow_version"] = Image.__version__
    _save("lpips_direct", out)
    sys.stdout.write(f"wrote lpips_direct.pt: ref_rel_dev {out['ref_rel_dev']:.3e}, names {out['state_dict_names']}\n")


def gen_runner(case):
    holder = {}

    def perceptual(R):
        holder["model"], holder["net"], holder["rec"] = real_perceptual(R)
        return holder["model"]

    def extra(R, stack):
        for name, cls in (("Resize", _Resize), ("ToTensor", _ToTensor), ("Normalize", _Normalize), ("Compose", _Compose)):
            stack.enter_context(mock.patch.object(R.Transforms, name, cls))
    del RESIZED[:]
    g = gvm.gen_case(case, perceptual=perceptual, extra=extra, save=False)
    old = load_golden(OUT, f"video_metrics_{case}.pt")
    lins, shift, scale = net_constants(holder["net"])
    backbone = lpips_ref.make_backbone(SEED)
    Cc = g["channels"]
    flat = torch.cat(holder["rec"]["values"])
    out = dict(case=case, seed=SEED, recipe=lpips_ref.RECIPE, probes=lpips_ref.backbone_probe(backbone), lins=lins, shift=shift, scale=scale,
               channels=Cc, preds_per_test=g["preds_per_test"], dataset=g["dataset"], config_name=g["config_name"], value={1: [], 2: []},
               value64={1: [], 2: []})
    pos, devs = 0, []
    n_iter = max(len(g["frames"][1]), len(g["frames"][2]))
    for it in range(n_iter):
        for ph in (1, 2):
            if it >= len(g["frames"][ph]):
                continue
            pred, real = g["frames"][ph][it]
            assert torch.equal(pred, old["frames"][ph][it][0]) and torch.equal(real, old["frames"][ph][it][1]), "frames differ from video_metrics"
            B, T = pred.shape[0], pred.shape[1] // Cc
            v = flat[pos:pos + B * T].reshape(B, T)
            pos += B * T
            v64, _, _ = lpips_ref.frame_lpips64(pred, real[:, :Cc * T], Cc, backbone, lins, shift, scale)
            devs.append(check_and_dev(v, v64, f"{case} phase {ph} batch {it}"))
            assert (v > 0).all()
            out["value"][ph].append(v)
            out["value64"][ph].append(v64)
    assert pos == flat.numel()
    out["vid_lpips"], out["vid_lpips2"] = g["vid_lpips_list"], g["vid_lpips2_list"] or None
    out["metric_arrays"], out["vid_metrics"] = g["metric_arrays"], g["vid_metrics"]
    assert out["vid_metrics"] is not None and "lpips" in out["vid_metrics"]
    out["ref_rel_dev"] = max(devs)
    _save(f"lpips_runner_{case}", out)
    sys.stdout.write(f"wrote lpips_runner_{case}.pt: ref_rel_dev {out['ref_rel_dev']:.3e}, lpips {out['vid_metrics']['lpips']}\n")


if __name__ == "__main__":
    torch.set_num_threads(4)
    for c in sys.argv[1:] or ["direct", "smmnist", "cityscapes"]:
        gen_direct() if c == "direct" else gen_runner(c)
