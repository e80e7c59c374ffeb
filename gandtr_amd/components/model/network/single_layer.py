"""Nets of one layer -- host mirror of mdir/components/model/network/single_layer.py:7-12 (torch ops on whatever device the input lives on)."""
from .cirnet import L2N


class NormalizationL2(L2N):
    """L2 normalisation of the input along dimension 1"""

    def __init__(self):
        super().__init__()
        self.meta = {}
