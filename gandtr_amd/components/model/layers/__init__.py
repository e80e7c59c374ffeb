"""Layers of the reference's mdir/components/model/layers that the retrieval embedders use: attention (L2NormAttention), pooling
(GeometricMedianWeiszfeld) and preprocessing (EdgeFilter)."""
from . import attention, pooling, preprocessing  # noqa: F401
