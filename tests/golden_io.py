"""Loading of the fixtures under tests/golden/ (tests only).

A committed file stays under 1 MiB, so a fixture whose tensors are larger keeps them in companion files: the value in the main
file is then {"parts": [file, ...], "dim": d}, and the tensor is torch.cat of the parts' tensors along d."""
import os

import torch


def load_golden(golden_dir, name):
    g = torch.load(os.path.join(golden_dir, name), weights_only=False)
    for k, v in list(g.items()):
        if isinstance(v, dict) and set(v) == {"parts", "dim"}:
            g[k] = torch.cat([torch.load(os.path.join(golden_dir, p), weights_only=True) for p in v["parts"]], v["dim"])
    return g
