"""mcvd_pytorch_amd: MI355X (gfx950) native MCVD sampling hot path.

Python host code keeping the reference's call surface (`scorenet(x, t, cond=)`, `ddpm_sampler`, `ddim_sampler`, the YAML
config schema) on top of hand-written HIP kernels reached through the C ABI of libmcvd_hip.so (include/mcvd_hip.h).
Importing this package loads the shared library and raises if it is missing -- there is no CPU or eager fallback.
"""
from . import _lib  # noqa: F401  (fails loudly when the HIP extension is not built)
from .config import desc_from_config, dict2namespace, load_config  # noqa: F401
from .samplers import ddim_sampler, ddpm_sampler, fpndm_sampler, get_sampler  # noqa: F401
from .scorenet import HipScoreNet, get_model  # noqa: F401
from .checkpoint import load_model, load_states_into  # noqa: F401
from .runner import (conditioning_fn, data_transform, evaluate_video_gen, fast_fid, frames_to_uint8, guidance_conditioning,  # noqa: F401
                     inverse_data_transform,
                     nearest_neighbors, sample, save_video_pred, stretch_image, task_conditioning, test_checkpoints, video_gen, video_gen_aliases,
                     video_tasks)
from .metrics import (FidInception, LpipsNet, NearestNeighbors, VideoMetrics, feature_stats, fid_from_features, fid_from_stats, fid_pr, frame_lpips,  # noqa: F401
                      frame_metrics, frechet_distance, fvd_clips, fvd_gates, knn_radii, knn_search, manifold_hits, precision_recall, video_lpips)
from .losses import anneal_dsm_score_estimation  # noqa: F401

__all__ = ["HipScoreNet", "get_model", "ddpm_sampler", "ddim_sampler", "fpndm_sampler", "get_sampler", "dict2namespace", "load_config",
           "desc_from_config", "load_model", "load_states_into", "conditioning_fn", "data_transform",
           "inverse_data_transform", "video_gen", "video_tasks", "task_conditioning", "guidance_conditioning", "save_video_pred", "frames_to_uint8",
           "frame_metrics", "VideoMetrics", "LpipsNet", "frame_lpips", "video_lpips", "anneal_dsm_score_estimation", "test_checkpoints",
           "fvd_gates", "fvd_clips", "feature_stats", "frechet_distance", "knn_radii", "manifold_hits", "precision_recall",
           "fid_from_features", "fid_from_stats", "fid_pr", "fast_fid", "knn_search", "FidInception",
           "NearestNeighbors", "nearest_neighbors", "evaluate_video_gen", "video_gen_aliases", "sample", "stretch_image"]
