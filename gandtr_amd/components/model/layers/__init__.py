"""Layers of the reference's mdir/components/model/layers that the retrieval embedders use: attention (L2NormAttention), pooling
(GeometricMedianWeiszfeld), preprocessing (EdgeFilter), and the grouping of local descriptors over codebooks (grouping, functional)."""
from . import attention, functional, grouping, pooling, preprocessing  # noqa: F401
