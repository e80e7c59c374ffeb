"""Attention layers -- host mirror of mdir/components/model/layers/attention.py:4-20.  On a HIP device the weights are computed by
csrc/pool_head.hip (pixel_norm_kernel) inside the descriptor head of CirRetrievalNetAttention."""
import torch.nn as nn


class L2NormAttention(nn.Module):
    """One weight per position of a 1 x D x H x W map: sqrt(sum_c x_c^2 + 1e-10), divided by its maximum when ``normalize_max``.  Like the reference's
    (its ``squeeze(0)`` drops the batch dimension) this is a layer for ONE image: the maximum is the image's."""

    def __init__(self, normalize_max):
        super().__init__()
        self.normalize_max = normalize_max

    def forward(self, x):
        m = (x.pow(2.0).sum(1) + 1e-10).sqrt().squeeze(0).squeeze(0)
        if self.normalize_max:
            m = m / m.max()
        return m


ATTENTIONS = {
    "l2norm": L2NormAttention,
}
