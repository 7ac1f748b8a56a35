"""The one-level ngf-288 nets of tests/golden/w288_forward.pt, shared by tools/gen_w288_golden.py, tests/test_w288_cpu.py and
tests/test_gpu_w288.py (not a test module).

`tiny` / `tiny_spade` with image_size 8, ngf 288, heads of 288 channels, ch_mult [4], one ResBlock per level and attention at 8: the smallest
net with everything the ngf-288 UCF-101 models add -- the time embedding at 288 (T = 1152; 1296 with cond_emb), 1152 + 1152 = 2304 -> 1152 at
8 x 8 with its 1x1 shortcut, 1152 + 288 = 1440 -> 1152, four heads of 288.  Weights are synth.make_state_dict(config, SEED), never stored.
"""
import os

import torch

from oracle import synth, unet_ref

SEED = 123
BATCH = 2
CASES = ("plain", "spade", "condemb")
FIXTURE = "w288_forward.pt"
TAP_STRIDE = 9            # the first up block's output [B, 1152, 8, 8] is stored as flat[::9] (coprime with 64: every pixel position and channel residue)


def make_config(case):
    config = synth.make_config("tiny_spade" if case == "spade" else "tiny")
    config.data.image_size = 8
    config.model.ngf = 288
    config.model.n_head_channels = 288
    config.model.ch_mult = [4]
    config.model.num_res_blocks = 1
    config.model.attn_resolutions = [8]
    if case == "spade":
        config.model.spade = True
        config.model.spade_dim = 64
    if case == "condemb":
        config.model.cond_emb = True
    return config


def first_up_block(config):
    """Index in all_modules of the first ResBlock of the up path: the one that reads the 2304-channel concat."""
    mods = unet_ref.module_plan(unet_ref.hot_cfg(config))
    idx = [i for i, m in enumerate(mods) if m["kind"] == "res" and m["cin"] == 2304]
    assert len(idx) == 1 and mods[idx[0]]["cout"] == 1152, idx
    assert any(m["kind"] == "res" and m["cin"] == 1440 for m in mods)
    return idx[0]


def load(golden_dir):
    return torch.load(os.path.join(golden_dir, FIXTURE), weights_only=False)
