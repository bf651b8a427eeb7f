"""bayesgm.utils.helpers -> bayesgm_amd.utils (the same objects)."""
from bayesgm_amd.utils import estimate_latent_dims, get_ADRF, get_SDR_dim, slice_y

__all__ = ["get_ADRF", "estimate_latent_dims", "get_SDR_dim", "slice_y"]
