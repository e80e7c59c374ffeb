"""Layers of the reference's mdir/components/model/layers that the retrieval embedders use: attention (L2NormAttention) and preprocessing (EdgeFilter)."""
from . import attention, preprocessing  # noqa: F401
