"""fp64 CPU restatement of the denoising score-matching loss (losses/dsm.py:37-52) and the parity gates of its tests (tests only).

Gates (one forward is within delta = 1e-4 max|eps_ref| of the reference, element by element).  With eps = eps_ref + e,
|e| <= delta, and the fixture's own z:
  L2: |1/2 (z - eps)^2 - 1/2 (z - eps_ref)^2| <= |z - eps_ref| delta + delta^2 / 2 per element, so per row
      |L_dev - L_ref| <= sum |z - eps_ref| delta + N delta^2 / 2 + 3 drift64 L_ref;
  L1: ||z - eps| - |z - eps_ref|| <= delta per element: |L_dev - L_ref| <= N delta + 3 drift64 L_ref;
drift64 = the reference's recorded fp32-vs-fp64 relative distance of the same call (its own rounding, which the device's fp64 sum does not
share); the mean gets the mean of the row gates."""
import torch


def loss_rows64(z, eps, L1=False):
    """Per-row sum of the terms in float64: 1/2 (z - eps)^2, or |z - eps|."""
    d = z.double() - eps.double()
    t = d.abs() if L1 else 0.5 * d.square()
    return t.reshape(len(z), -1).sum(dim=-1)


def terms32_sum64(z, eps, L1=False):
    """The device's definition: the fp32 terms the reference forms (d = z - eps, 0.5 * d * d or |d|, all fp32), summed in fp64."""
    d = z.float() - eps.float()
    t = d.abs() if L1 else 0.5 * (d * d)
    return t.double().reshape(len(z), -1).sum(dim=-1)


def perturb32(x, labels, alphas, z):
    """losses/dsm.py:37 in torch fp32: sqrt(a) x + sqrt(1 - a) z."""
    a = alphas[labels].reshape(len(x), *([1] * (x.dim() - 1)))
    return a.sqrt() * x + (1 - a).sqrt() * z


def row_gates(z, eps_ref, L_ref, drift64, L1=False):
    """Per-row bound on |L_dev - L_ref| (module docstring).  drift64: one number (the recorded distance of the call)."""
    z, eps_ref, L_ref = z.double(), eps_ref.double(), L_ref.double()
    delta = 1e-4 * eps_ref.abs().max().item()
    N = z[0].numel()
    if L1:
        g = torch.full_like(L_ref, N * delta)
    else:
        g = (z - eps_ref).abs().reshape(len(z), -1).sum(dim=-1) * delta + 0.5 * N * delta * delta
    return g + 3 * drift64 * L_ref.abs()
