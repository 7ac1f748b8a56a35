"""Golden vectors of the FID InceptionV3 as the REAL reference runs it -- build container only (needs the reference checkout).

    PYTHONDONTWRITEBYTECODE=1 python -m tools.gen_fid_inception_golden

The real `evaluation/inception.py` is imported and its real `InceptionV3([0, 1, 2, 3])` and `InceptionV3([3])` are run on the CPU: the
block structure (:84-124), the forward (:129-163), `fid_inception_v3` (:184-208) and the four patched forwards (:211-328) are the
reference's own code.  Replaced from the outside, nothing else (the construction of tools/gen_lpips_golden.py):
  * `torchvision` -> a stand-in registered in sys.modules before the import (torchvision is not installed here): `__version__`,
    `models.inception_v3(num_classes, aux_logits, pretrained, init_weights)` and `models.inception.InceptionA/B/C/D/E` / `BasicConv2d`,
    written from the published architecture (constructors, and the forwards of B and D which the FID variant does not patch);
  * `load_state_dict_from_url` of that module -> a function that returns the SEEDED dict of tests/inception_ref.py (make_state_dict, one
    generator per tensor).  Nothing attempts a download.  The 87 MB of weights are not stored: the fixture keeps the seed, the recipe and
    per tensor its fp64 sum and 64 probed values.

tests/golden/fid_inception.pt:
    seed, recipe, probes {name: (fp64 sum, 64 values)}, state_dict_names (of the real patched torchvision-shaped module, fc and
    num_batches_tracked included), images_64 [3, 3, 64, 64], images_40x56 [2, 3, 40, 56], image_299 = (name, shape, probe) of the seeded
    299 x 299 image, sets [(key, n)], block3 {key: fp32 [n, 2048, 1, 1]} in full, block_probes {key: [block 0..2][image] (fp64 sum, 64
    values)}, block{0,1,2}_image0 (the first 64 x 64 image's block outputs in full), block3_only (InceptionV3([3]) on images_64),
    ref_rel_dev [4] = max |real fp32 - fp64 restatement| / max |fp64| per block over all sets, stats [4] (mean |x|, share of zeros);
    resize {size key: dict(name, shape, probe, rel_dev)}, resize_stripe (indices 0, 8, ...), resize_rows_<key> [1, 1, len(stripe), 299] and
    resize_cols_<key> [1, 1, 299, len(stripe)]: torch's own F.interpolate(..., 299) then 2 x - 1 in fp32 of the seeded one-channel image
    on two stripes that between them touch every row and every column, and its deviation from the same calls in fp64 (whole image).
Nothing is written unless every block output is finite, has mean |x| in [1e-2, 1e2] and fewer than 60 % exact zeros, and block-3 rows of
different images differ by more than 0.1 (conditions on the inputs, not tolerances).
"""
import importlib.util
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from oracle.gen_runner_golden import REF  # noqa: E402
from tests import inception_ref as ir  # noqa: E402
from tools.gen_video_tasks_golden import _save  # noqa: E402

SEED = 11
BUILT = []      # the torchvision-shaped modules the stand-in built, in order


class BasicConv2d(nn.Module):
    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, bias=False, **kwargs)
        self.bn = nn.BatchNorm2d(out_channels, eps=0.001)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)), inplace=True)


class InceptionA(nn.Module):
    def __init__(self, in_channels, pool_features):
        super().__init__()
        self.branch1x1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(in_channels, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(in_channels, pool_features, kernel_size=1)


class InceptionB(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch3x3 = BasicConv2d(in_channels, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)

    def forward(self, x):
        branch3x3 = self.branch3x3(x)
        branch3x3dbl = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        branch_pool = F.max_pool2d(x, kernel_size=3, stride=2)
        return torch.cat([branch3x3, branch3x3dbl, branch_pool], 1)


class InceptionC(nn.Module):
    def __init__(self, in_channels, channels_7x7):
        super().__init__()
        c7 = channels_7x7
        self.branch1x1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(in_channels, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(in_channels, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(in_channels, 192, kernel_size=1)


class InceptionD(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)

    def forward(self, x):
        branch3x3 = self.branch3x3_2(self.branch3x3_1(x))
        branch7x7x3 = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        branch_pool = F.max_pool2d(x, kernel_size=3, stride=2)
        return torch.cat([branch3x3, branch7x7x3, branch_pool], 1)


class InceptionE(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch1x1 = BasicConv2d(in_channels, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(in_channels, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(in_channels, 192, kernel_size=1)


class Inception3(nn.Module):
    """The members evaluation/inception.py takes (:84-124) and load_state_dict fills, in torchvision's order; no forward of its own is
    called by the reference."""

    def __init__(self, num_classes=1000, aux_logits=True):
        super().__init__()
        assert not aux_logits, "the FID variant is built with aux_logits=False"
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.Mixed_5b = InceptionA(192, pool_features=32)
        self.Mixed_5c = InceptionA(256, pool_features=64)
        self.Mixed_5d = InceptionA(288, pool_features=64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, channels_7x7=128)
        self.Mixed_6c = InceptionC(768, channels_7x7=160)
        self.Mixed_6d = InceptionC(768, channels_7x7=160)
        self.Mixed_6e = InceptionC(768, channels_7x7=192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280)
        self.Mixed_7c = InceptionE(2048)
        self.fc = nn.Linear(2048, num_classes)


def inception_v3(num_classes=1000, aux_logits=True, pretrained=False, init_weights=None):
    assert not pretrained, "nothing is downloaded"
    BUILT.append(Inception3(num_classes=num_classes, aux_logits=aux_logits))
    return BUILT[-1]


def import_real_inception():
    tv = types.ModuleType("torchvision")
    tv.__version__ = "0.15.0"
    tv.models = types.ModuleType("torchvision.models")
    tv.models.inception_v3 = inception_v3
    tv.models.inception = types.ModuleType("torchvision.models.inception")
    for cls in (BasicConv2d, InceptionA, InceptionB, InceptionC, InceptionD, InceptionE):
        setattr(tv.models.inception, cls.__name__, cls)
    assert "torchvision" not in sys.modules, "a real torchvision is installed: use it instead of the stand-in"
    sys.modules.update({"torchvision": tv, "torchvision.models": tv.models, "torchvision.models.inception": tv.models.inception})
    spec = importlib.util.spec_from_file_location("real_fid_inception", os.path.join(REF, "evaluation", "inception.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.load_state_dict_from_url = lambda url, progress=True: ir.make_state_dict(SEED, fc=True)
    return mod


def resize_case(x):
    """torch's own resize + 2 x - 1 in fp32 and fp64 on two stripes covering every row and every column."""
    y32 = 2 * F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False) - 1
    y64 = 2 * F.interpolate(x.double(), size=(299, 299), mode="bilinear", align_corners=False) - 1
    rows = torch.arange(0, 299, 8)
    return dict(rows=rows, row_values=y32[:, :, rows].clone(), col_values=y32[:, :, :, rows].clone(), rel_dev=ir.rel_dev(y32, y64))


def main():
    torch.set_num_threads(8)
    mod = import_real_inception()
    with torch.no_grad():
        real_all = mod.InceptionV3([0, 1, 2, 3]).eval()
        real_3 = mod.InceptionV3([3]).eval()
    assert len(BUILT) == 2
    sd = ir.make_state_dict(SEED)
    name299, shape299 = "image_299", (1, 3, 299, 299)
    sets = [("images_64", ir.make_images(SEED, "images_64", (3, 3, 64, 64))),
            ("images_40x56", ir.make_images(SEED, "images_40x56", (2, 3, 40, 56))),
            (name299, ir.make_images(SEED, name299, shape299))]
    out = dict(seed=SEED, recipe=ir.RECIPE, probes=ir.probe(sd), state_dict_names=list(BUILT[0].state_dict().keys()),
               images_64=sets[0][1], images_40x56=sets[1][1], image_299=(name299, shape299, ir.probe_tensor(sets[2][1])),
               sets=[(k, len(v)) for k, v in sets], block3={}, block_probes={})
    devs, absmean, zeros, nel = [0.0] * 4, [0.0] * 4, [0.0] * 4, [0] * 4
    rows3 = []
    for key, x in sets:
        with torch.no_grad():
            real = real_all(x)
        want = ir.forward(sd, x, torch.float64)
        assert len(real) == 4
        for b in range(4):
            assert real[b].dtype == torch.float32 and real[b].shape == want[b].shape and real[b].shape[1] == ir.BLOCK_CHANNELS[b]
            assert torch.isfinite(real[b]).all(), f"{key}: block {b} is not finite"
            devs[b] = max(devs[b], ir.rel_dev(real[b], want[b]))
            absmean[b] += real[b].abs().double().sum().item()
            zeros[b] += (real[b] == 0).sum().item()
            nel[b] += real[b].numel()
            m, z = real[b].abs().mean().item(), (real[b] == 0).double().mean().item()
            assert 1e-2 <= m <= 1e2 and z < 0.6, f"{key}: block {b} has mean |x| {m:.3g} and {z:.2f} zeros"
        out["block3"][key] = real[3].clone()
        out["block_probes"][key] = [[ir.probe_tensor(real[b][i]) for i in range(len(x))] for b in range(3)]
        rows3.append(real[3].reshape(len(x), -1))
        if key == "images_64":
            for b in range(3):
                out[f"block{b}_image0"] = real[b][0].clone()
            with torch.no_grad():
                only = real_3(x)
            assert len(only) == 1 and torch.equal(only[0], real[3])
            out["block3_only"] = only[0].clone()
    rows3 = torch.cat(rows3)
    d = torch.cdist(rows3.double(), rows3.double()) + 1e9 * torch.eye(len(rows3))
    assert d.min().item() > 0.1, f"two images have block-3 rows only {d.min().item():.3g} apart"
    assert max(devs) < 1e-4, f"the restatement is {max(devs):.3e} away from the real module: not the same function"
    out["ref_rel_dev"] = devs
    out["stats"] = [(absmean[b] / nel[b], zeros[b] / nel[b]) for b in range(4)]
    out["resize"] = {}
    for key, shape in (("32", (1, 1, 32, 32)), ("64", (1, 1, 64, 64)), ("40x56", (1, 1, 40, 56)), ("299", (1, 1, 299, 299)),
                       ("300", (1, 1, 300, 300))):
        x = ir.make_images(SEED, "resize_" + key, shape)
        c = resize_case(x)
        out["resize"][key] = dict(name="resize_" + key, shape=shape, probe=ir.probe_tensor(x), rel_dev=c["rel_dev"])
        out["resize_stripe"] = c["rows"]
        out[f"resize_rows_{key}"], out[f"resize_cols_{key}"] = c["row_values"], c["col_values"]
        if key == "299":
            assert torch.equal(c["row_values"], 2 * x[:, :, c["rows"]] - 1), "torch's 299 -> 299 resize is not the identity"
    _save("fid_inception", out)
    sys.stdout.write("wrote fid_inception.pt: ref_rel_dev %s, stats %s, resize rel_dev %s, %d keys\n"
                     % (["%.2e" % v for v in devs], [("%.2f" % a, "%.2f" % z) for a, z in out["stats"]],
                        {k: "%.2e" % v["rel_dev"] for k, v in out["resize"].items()}, len(out["state_dict_names"])))


if __name__ == "__main__":
    main()
