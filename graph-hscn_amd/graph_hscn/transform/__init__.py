from .posenc import compute_posenc_stats, eigvec_normalizer, get_lap_decomp_stats
from .pre_transform import pre_transform_in_memory

__all__ = ["compute_posenc_stats", "eigvec_normalizer", "get_lap_decomp_stats", "pre_transform_in_memory"]
