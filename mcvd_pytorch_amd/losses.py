"""The denoising score-matching (DSM) loss of `NCSNRunner.test()` on the device: `anneal_dsm_score_estimation` (losses/dsm.py:7-52) with the
perturbation, the UNet forward and the per-row reduction in one C ABI call (mcvd_dsm_loss, kernels/dsm.cpp).  Forward only: no gradients,
no optimiser -- training stays out of scope.
"""
import ctypes as C

import torch

from . import _lib
from .samplers import _draw_seed, _unwrap


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@torch.no_grad()
def dsm_loss_rows(scorenet, x, labels, cond=None, cond_mask=None, gamma=False, L1=False, z=None, seed=None, sample_offset=0,
                  return_z=False, return_perturbed=False):
    """Per-row DSM losses [B] (fp32, on the net's device) of x [B, C*nf, S, S] at `labels` [B] -> (loss_rows, z, perturbed_x), the last
    two None unless asked for.

      * z: None draws it on the device (Philox keyed by (seed, sample_offset + row): a row's z does not depend on the batch it is
        evaluated in; `seed` defaults to a draw from torch's CPU generator, so torch.manual_seed controls it); else the caller's
        tensor like x -- under `gamma` the RAW draw g of Gamma(k_cum[t], rate 1 / theta_t[t]), standardised on the device as
        (g - k theta) / sqrt(1 - alpha) (losses/dsm.py:31-34);
      * a noise_in_cond net draws its conditioning noise as its forward does (HipScoreNet.set_next_cond_noise injects it);
      * cond_mask reaches the forward of a model.cond_emb net (losses/dsm.py:47), as HipScoreNet.__call__ passes it."""
    net = _unwrap(scorenet)
    d = net._desc
    shape = (d.channels * d.num_frames, d.image_size, d.image_size)
    if x.dim() != 4 or tuple(x.shape[1:]) != shape:
        raise RuntimeError(f"x has shape {tuple(x.shape)}, the network takes [B, {shape[0]}, {shape[1]}, {shape[2]}]")
    B = x.shape[0]
    if labels.shape != (B,):
        raise RuntimeError(f"labels have shape {tuple(labels.shape)}, expected ({B},)")
    if labels.is_floating_point():
        raise IndexError("tensors used as indices must be long, int, byte or bool tensors (losses/dsm.py:29 indexes alphas with the labels)")
    if d.num_frames_cond > 0:
        if cond is None or tuple(cond.shape) != (B, d.channels * d.num_frames_cond, d.image_size, d.image_size):
            raise RuntimeError("cond missing or mis-shaped")
    elif cond is not None:
        raise RuntimeError("this model takes no conditioning frames (num_frames_cond == 0) but cond was passed")
    if z is not None and tuple(z.shape) != tuple(x.shape):
        raise RuntimeError(f"z has shape {tuple(z.shape)}, x {tuple(x.shape)}")
    if gamma and not getattr(net, "gamma", False):
        raise AttributeError("'HipScoreNet' object has no attribute 'k_cum' (gamma=True needs a model.gamma net, losses/dsm.py:31)")
    if net.plan_only:
        raise RuntimeError("HipScoreNet(plan_only=True) cannot compute (no GPU context)")
    net.sync_parameters()
    dev = net.device
    x = net._prep(x.to(dev), "x")
    cond = net._prep(cond.to(dev), "cond") if cond is not None else None
    y = labels.to(device=dev, dtype=torch.int64).contiguous()
    zin = net._prep(z.to(dev), "z") if z is not None else None
    mask = None
    if d.cond_emb and cond_mask is not None:
        mask = cond_mask.to(device=dev, dtype=torch.int32).contiguous()
        if mask.shape != (B,):
            raise RuntimeError(f"cond_mask has shape {tuple(mask.shape)}")
    if zin is None and seed is None:
        seed = _draw_seed()
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    z_out = torch.empty_like(x) if return_z else None
    px_out = torch.empty_like(x) if return_perturbed else None
    flags = (_lib.DSM_L1 if L1 else 0) | (_lib.DSM_GAMMA if gamma else 0)
    with torch.cuda.device(dev):
        net._bind_stream()
        nic = net.noise_in_cond and cond is not None
        zc = net._arm_cond_noise(cond, y) if nic else None      # noqa: F841 -- kept alive until the call is enqueued
        if d.spade:
            # the forward recomputes the SPADE maps of this cond (a cached (pointer, batch) from an earlier call may hold other frames)
            _lib.check(_lib.lib.mcvd_model_invalidate_cond(net._model))
            net._cond_key = None
        try:
            rc = _lib.lib.mcvd_dsm_loss(net._model, _ptr(x), _ptr(y), _ptr(cond), _ptr(mask), _ptr(zin), C.c_uint64(int(seed or 0)),
                                        C.c_uint64(int(sample_offset)), flags, _ptr(loss), _ptr(z_out), _ptr(px_out), B)
        finally:
            if nic:
                _lib.lib.mcvd_model_set_cond_noise(net._model, None, 0, 0, 0)
        _lib.check(rc, "dsm_loss")
    return loss, z_out, px_out


@torch.no_grad()
def anneal_dsm_score_estimation(scorenet, x, labels=None, loss_type='a', hook=None, cond=None, cond_mask=None, gamma=False, L1=False,
                                all_frames=False, z=None, seed=None, sample_offset=0):
    """losses/dsm.py:7-52 with the reference's signature and result: the 0-dim fp32 mean over rows of the per-row losses
    sum 1/2 (z - eps)^2 (or sum |z - eps| with L1), `hook(loss_rows, labels)` called with the per-row tensor first.

      * labels: torch.randint(0, len(alphas), (B,), device=x.device) as the reference draws them (:27-28);
      * z: drawn on the device (dsm_loss_rows) -- `z=` / `seed=` / `sample_offset=` override the draw for parity runs and sharding,
        as the samplers take noise= / seed= / sample_offset=; under `gamma` an injected z is the raw Gamma draw;
      * version SMLD (sigma-perturbed, :18-24) raises NotImplementedError: the SMLD samplers are out of scope;
      * all_frames=True raises the error the reference hits (:13-15: x gains the cond channels, the net returns C*nf of them and
        `z - eps` cannot broadcast), before any device work.  `loss_type` is accepted and unused, as in the reference."""
    net = scorenet.module if hasattr(scorenet, "module") else scorenet
    version = getattr(net, "version", "SMLD").upper()
    if version == "SMLD":
        raise NotImplementedError("anneal_dsm_score_estimation: the SMLD (sigma-perturbed) version is out of scope (DESIGN section 8)")
    if version not in ("DDPM", "DDIM", "FPNDM"):
        raise NotImplementedError(f"anneal_dsm_score_estimation: version {version!r} has no perturbation in the reference either")
    if all_frames:
        full = torch.cat([x, cond], dim=1)                  # :14 (a None cond fails here as in the reference)
        out_ch = net._desc.channels * net._desc.num_frames
        raise RuntimeError(f"The size of tensor a ({full.shape[1]}) must match the size of tensor b ({out_ch}) at non-singleton dimension 1")
    if labels is None:
        labels = torch.randint(0, len(net.alphas), (x.shape[0],), device=x.device)
    loss, _, _ = dsm_loss_rows(net, x, labels, cond=cond, cond_mask=cond_mask, gamma=gamma, L1=L1, z=z, seed=seed,
                               sample_offset=sample_offset)
    if hook is not None:
        hook(loss, labels)
    return loss.mean(dim=0)
