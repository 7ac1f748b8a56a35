"""Restatement of the FID InceptionV3 (evaluation/inception.py) as a table of its 94 conv + BN + ReLU layers and one functional forward in
any dtype, with no torchvision, so that it runs wherever the tests run.  Besides the kernels (csrc/kernels/inception.cpp) this is the one
place the net is written down.

  * InceptionV3.forward (evaluation/inception.py:129-163): F.interpolate(size=(299, 299), mode='bilinear', align_corners=False) when
    resize_input, 2 x - 1 when normalize_input, then the blocks of :84-124 -- block 0 Conv2d_1a_3x3, Conv2d_2a_3x3, Conv2d_2b_3x3,
    MaxPool2d(3, 2); block 1 Conv2d_3b_1x1, Conv2d_4a_3x3, MaxPool2d(3, 2); block 2 Mixed_5b ... Mixed_6e; block 3 Mixed_7a, Mixed_7b,
    Mixed_7c, AdaptiveAvgPool2d((1, 1)).
  * Every named layer is torchvision's BasicConv2d: Conv2d(bias=False), BatchNorm2d(eps=0.001) in eval mode, ReLU.
  * Mixed_5b/5c/5d: FIDInceptionA.forward (:216-233); Mixed_6b..6e: FIDInceptionC.forward (:241-261); Mixed_7b: FIDInceptionE_1.forward
    (:269-294); Mixed_7c: FIDInceptionE_2.forward (:302-328, a MAX pool in the pool branch).  Their avg_pool2d calls are
    count_include_pad=False.  Mixed_6a and Mixed_7a are torchvision's InceptionB and InceptionD (a MaxPool2d(3, 2) branch), which the FID
    variant does not patch (:196-204).

The weights of the tests are seeded (make_state_dict): whether the computation is right does not depend on which weights are loaded, and
the 87 MB are never stored -- fixtures keep the seed, the recipe and per tensor a probe (probe()).
"""
import torch
import torch.nn.functional as F

from oracle import synth

SIZE = 299
BN_EPS = 0.001
BLOCK_CHANNELS = (64, 192, 768, 2048)
RECIPE = ("conv.weight randn*sqrt(2/fan_in); bn.weight 0.5+rand; bn.running_var 0.5+rand; bn.bias 0.1*randn; bn.running_mean 0.1*randn; "
          "generator oracle.synth._gen(seed, '<layer>.conv.weight|bn.weight|bn.bias|bn.running_mean|bn.running_var')")


def _inception_a(p, cin, pool_features):
    return [(p + ".branch1x1", cin, 64, 1, 1, 1, 0, 0), (p + ".branch5x5_1", cin, 48, 1, 1, 1, 0, 0), (p + ".branch5x5_2", 48, 64, 5, 5, 1, 2, 2),
            (p + ".branch3x3dbl_1", cin, 64, 1, 1, 1, 0, 0), (p + ".branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1),
            (p + ".branch3x3dbl_3", 96, 96, 3, 3, 1, 1, 1), (p + ".branch_pool", cin, pool_features, 1, 1, 1, 0, 0)]


def _inception_b(p, cin):
    return [(p + ".branch3x3", cin, 384, 3, 3, 2, 0, 0), (p + ".branch3x3dbl_1", cin, 64, 1, 1, 1, 0, 0),
            (p + ".branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1), (p + ".branch3x3dbl_3", 96, 96, 3, 3, 2, 0, 0)]


def _inception_c(p, cin, c7):
    return [(p + ".branch1x1", cin, 192, 1, 1, 1, 0, 0), (p + ".branch7x7_1", cin, c7, 1, 1, 1, 0, 0), (p + ".branch7x7_2", c7, c7, 1, 7, 1, 0, 3),
            (p + ".branch7x7_3", c7, 192, 7, 1, 1, 3, 0), (p + ".branch7x7dbl_1", cin, c7, 1, 1, 1, 0, 0),
            (p + ".branch7x7dbl_2", c7, c7, 7, 1, 1, 3, 0), (p + ".branch7x7dbl_3", c7, c7, 1, 7, 1, 0, 3),
            (p + ".branch7x7dbl_4", c7, c7, 7, 1, 1, 3, 0), (p + ".branch7x7dbl_5", c7, 192, 1, 7, 1, 0, 3),
            (p + ".branch_pool", cin, 192, 1, 1, 1, 0, 0)]


def _inception_d(p, cin):
    return [(p + ".branch3x3_1", cin, 192, 1, 1, 1, 0, 0), (p + ".branch3x3_2", 192, 320, 3, 3, 2, 0, 0),
            (p + ".branch7x7x3_1", cin, 192, 1, 1, 1, 0, 0), (p + ".branch7x7x3_2", 192, 192, 1, 7, 1, 0, 3),
            (p + ".branch7x7x3_3", 192, 192, 7, 1, 1, 3, 0), (p + ".branch7x7x3_4", 192, 192, 3, 3, 2, 0, 0)]


def _inception_e(p, cin):
    return [(p + ".branch1x1", cin, 320, 1, 1, 1, 0, 0), (p + ".branch3x3_1", cin, 384, 1, 1, 1, 0, 0),
            (p + ".branch3x3_2a", 384, 384, 1, 3, 1, 0, 1), (p + ".branch3x3_2b", 384, 384, 3, 1, 1, 1, 0),
            (p + ".branch3x3dbl_1", cin, 448, 1, 1, 1, 0, 0), (p + ".branch3x3dbl_2", 448, 384, 3, 3, 1, 1, 1),
            (p + ".branch3x3dbl_3a", 384, 384, 1, 3, 1, 0, 1), (p + ".branch3x3dbl_3b", 384, 384, 3, 1, 1, 1, 0),
            (p + ".branch_pool", cin, 192, 1, 1, 1, 0, 0)]


# (name, Cin, Cout, kh, kw, stride, pad_h, pad_w), in torchvision's module order
LAYERS = tuple(
    [("Conv2d_1a_3x3", 3, 32, 3, 3, 2, 0, 0), ("Conv2d_2a_3x3", 32, 32, 3, 3, 1, 0, 0), ("Conv2d_2b_3x3", 32, 64, 3, 3, 1, 1, 1),
     ("Conv2d_3b_1x1", 64, 80, 1, 1, 1, 0, 0), ("Conv2d_4a_3x3", 80, 192, 3, 3, 1, 0, 0)]
    + _inception_a("Mixed_5b", 192, 32) + _inception_a("Mixed_5c", 256, 64) + _inception_a("Mixed_5d", 288, 64)
    + _inception_b("Mixed_6a", 288)
    + _inception_c("Mixed_6b", 768, 128) + _inception_c("Mixed_6c", 768, 160) + _inception_c("Mixed_6d", 768, 160)
    + _inception_c("Mixed_6e", 768, 192)
    + _inception_d("Mixed_7a", 768) + _inception_e("Mixed_7b", 1280) + _inception_e("Mixed_7c", 2048))
BY_NAME = {L[0]: L for L in LAYERS}
BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def param_names():
    """The keys FidInception needs, in torchvision's state_dict order (without num_batches_tracked and fc)."""
    out = []
    for L in LAYERS:
        out.append(L[0] + ".conv.weight")
        out.extend(f"{L[0]}.bn.{k}" for k in BN_KEYS)
    return out


def make_state_dict(seed, fc=False):
    """Seeded stand-in for pt_inception-2015-12-05-6726825d.pth, by its own key names: one generator per tensor.  fc: also the 1008-way
    classifier the real module's load_state_dict asks for (never used by the forward)."""
    sd = {}
    for name, cin, cout, kh, kw, _, _, _ in LAYERS:
        fan_in = cin * kh * kw
        sd[f"{name}.conv.weight"] = torch.randn((cout, cin, kh, kw), generator=synth._gen(seed, f"{name}.conv.weight")) * (2.0 / fan_in) ** 0.5
        sd[f"{name}.bn.weight"] = 0.5 + torch.rand((cout,), generator=synth._gen(seed, f"{name}.bn.weight"))
        sd[f"{name}.bn.bias"] = 0.1 * torch.randn((cout,), generator=synth._gen(seed, f"{name}.bn.bias"))
        sd[f"{name}.bn.running_mean"] = 0.1 * torch.randn((cout,), generator=synth._gen(seed, f"{name}.bn.running_mean"))
        sd[f"{name}.bn.running_var"] = 0.5 + torch.rand((cout,), generator=synth._gen(seed, f"{name}.bn.running_var"))
    if fc:
        sd["fc.weight"] = torch.randn((1008, 2048), generator=synth._gen(seed, "fc.weight")) * (1.0 / 2048) ** 0.5
        sd["fc.bias"] = torch.zeros(1008)
    return sd


def probe_tensor(v):
    """(fp64 sum, 64 probed values at fixed strides) of one tensor."""
    flat = v.reshape(-1)
    idx = torch.linspace(0, flat.numel() - 1, 64).long()
    return float(flat.double().sum()), flat[idx].clone()


def probe(sd):
    """name -> (fp64 sum, 64 probed values): what the fixture stores instead of the 87 MB of weights."""
    return {k: probe_tensor(v) for k, v in sd.items()}


def make_images(seed, name, shape):
    """Seeded images in [0, 1]: smooth blobs plus noise, so that neighbouring pixels differ and the resize has something to do."""
    g = synth._gen(seed, name)
    n, c, h, w = shape
    low = F.interpolate(torch.rand((n, c, max(h // 8, 2), max(w // 8, 2)), generator=g), size=(h, w), mode="bilinear", align_corners=False)
    return (0.7 * low + 0.3 * torch.rand(shape, generator=g)).clamp(0, 1)


def basic_conv(sd, name, x):
    """torchvision's BasicConv2d.forward in x's dtype: conv (no bias), eval-mode BatchNorm2d(eps=0.001), ReLU."""
    _, _, _, _, _, stride, ph, pw = BY_NAME[name]
    dt = x.dtype
    y = F.conv2d(x, sd[name + ".conv.weight"].to(dt), None, stride=stride, padding=(ph, pw))
    y = F.batch_norm(y, sd[name + ".bn.running_mean"].to(dt), sd[name + ".bn.running_var"].to(dt), sd[name + ".bn.weight"].to(dt),
                     sd[name + ".bn.bias"].to(dt), False, 0.0, BN_EPS)
    return F.relu(y)


def _avg(x):
    return F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False)


def inception_a(sd, p, x):      # evaluation/inception.py:216-233
    c = lambda n, v: basic_conv(sd, f"{p}.{n}", v)      # noqa: E731
    b5 = c("branch5x5_2", c("branch5x5_1", x))
    b3 = c("branch3x3dbl_3", c("branch3x3dbl_2", c("branch3x3dbl_1", x)))
    return torch.cat([c("branch1x1", x), b5, b3, c("branch_pool", _avg(x))], 1)


def inception_b(sd, p, x):      # torchvision InceptionB
    c = lambda n, v: basic_conv(sd, f"{p}.{n}", v)      # noqa: E731
    b3 = c("branch3x3dbl_3", c("branch3x3dbl_2", c("branch3x3dbl_1", x)))
    return torch.cat([c("branch3x3", x), b3, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


def inception_c(sd, p, x):      # evaluation/inception.py:241-261
    c = lambda n, v: basic_conv(sd, f"{p}.{n}", v)      # noqa: E731
    b7 = c("branch7x7_3", c("branch7x7_2", c("branch7x7_1", x)))
    bd = x
    for k in range(1, 6):
        bd = c(f"branch7x7dbl_{k}", bd)
    return torch.cat([c("branch1x1", x), b7, bd, c("branch_pool", _avg(x))], 1)


def inception_d(sd, p, x):      # torchvision InceptionD
    c = lambda n, v: basic_conv(sd, f"{p}.{n}", v)      # noqa: E731
    b3 = c("branch3x3_2", c("branch3x3_1", x))
    b7 = x
    for k in range(1, 5):
        b7 = c(f"branch7x7x3_{k}", b7)
    return torch.cat([b3, b7, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


def inception_e(sd, p, x, max_pool):      # evaluation/inception.py:269-294 (E_1, average) and :302-328 (E_2, max)
    c = lambda n, v: basic_conv(sd, f"{p}.{n}", v)      # noqa: E731
    b3 = c("branch3x3_1", x)
    b3 = torch.cat([c("branch3x3_2a", b3), c("branch3x3_2b", b3)], 1)
    bd = c("branch3x3dbl_2", c("branch3x3dbl_1", x))
    bd = torch.cat([c("branch3x3dbl_3a", bd), c("branch3x3dbl_3b", bd)], 1)
    pooled = F.max_pool2d(x, kernel_size=3, stride=1, padding=1) if max_pool else _avg(x)
    return torch.cat([c("branch1x1", x), b3, bd, c("branch_pool", pooled)], 1)


def net_input(images01, dtype=torch.float32, resize_input=True, normalize_input=True):
    """evaluation/inception.py:146-153 in `dtype`."""
    x = images01.to(dtype)
    if resize_input:
        x = F.interpolate(x, size=(SIZE, SIZE), mode="bilinear", align_corners=False)
    if normalize_input:
        x = 2 * x - 1
    return x


@torch.no_grad()
def forward(sd, images01, dtype=torch.float32, resize_input=True, normalize_input=True, last_block=3):
    """-> the outputs of blocks 0 .. last_block ([n, 64, ., .], [n, 192, ., .], [n, 768, ., .], [n, 2048, 1, 1]) in `dtype`."""
    x = net_input(images01, dtype, resize_input, normalize_input)
    out = []
    for name in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
        x = basic_conv(sd, name, x)
    x = F.max_pool2d(x, kernel_size=3, stride=2)
    out.append(x)
    if last_block >= 1:
        x = basic_conv(sd, "Conv2d_4a_3x3", basic_conv(sd, "Conv2d_3b_1x1", x))
        x = F.max_pool2d(x, kernel_size=3, stride=2)
        out.append(x)
    if last_block >= 2:
        for p in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
            x = inception_a(sd, p, x)
        x = inception_b(sd, "Mixed_6a", x)
        for p in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = inception_c(sd, p, x)
        out.append(x)
    if last_block >= 3:
        x = inception_d(sd, "Mixed_7a", x)
        x = inception_e(sd, "Mixed_7b", x, max_pool=False)
        x = inception_e(sd, "Mixed_7c", x, max_pool=True)
        out.append(F.adaptive_avg_pool2d(x, (1, 1)))
    return out


def rel_dev(got, want64):
    """max |got - want| / max |want|: the measure of every ref_rel_dev and of every gate built on one."""
    return ((got.double() - want64).abs().max() / want64.abs().max()).item()
