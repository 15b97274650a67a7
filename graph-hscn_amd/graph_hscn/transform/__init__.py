from .posenc import (compute_posenc_stats, compute_posenc_stats_batched, compute_posenc_stats_device, eigvec_normalizer,
                     get_lap_decomp_stats)
from .pre_transform import pre_transform_in_memory
from .rwse import compute_rwse_stats, compute_rwse_stats_device

__all__ = ["compute_posenc_stats", "compute_posenc_stats_batched", "compute_posenc_stats_device", "eigvec_normalizer", "get_lap_decomp_stats", "pre_transform_in_memory", "compute_rwse_stats", "compute_rwse_stats_device"]
