"""Pooling layers -- host mirror of mdir/components/model/layers/pooling.py:44-101 (GeometricMedianWeiszfeld, WeightedGeometricMedianWeiszfeld, POOLINGS).
On a HIP device the iteration runs in csrc/median_pool.hip (engine.geometric_median): one read of the map per iteration.

The reference's forward only works on a batch of one once ``iterations`` >= 1 (after the first iteration its weights are N x H x W, which ``x * weights``
cannot broadcast for N > 1, and ``weights.sum()`` would couple the images).  What is reproduced here, on the torch and on the HIP path, is that batch-of-one
forward applied to each image: a batch equals its images run one by one, bit for bit.  ``HordeCascadedKOrder`` is not mirrored: it returns a list, which
``ImageRetrievalNet.forward`` (``self.norm(self.pool(o))``) cannot take in the reference itself."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import attention as attention_layers


def weiszfeld(x, iterations, prior=None):
    """The geometric median of the positions of ONE image (1 x C x H x W -> 1 x C x 1 x 1) by Weiszfeld's iteration, in the reference's fp32 op sequence:
    m = sum_i w_i x_i / sum_i w_i, w_i = a_i / sqrt(|x_i - m|^2 + 1e-10), starting from w = a (``prior``, H x W; None: ones); 0 iterations: the mean"""
    size = (x.size(-2), x.size(-1))
    a = prior if prior is not None else torch.ones((1,) + size, device=x.device)
    w = a
    for _ in range(iterations):
        m = F.avg_pool2d(x * w, size, divisor_override=1) / w.sum()
        w = a / ((x - m).pow(2.0).sum(1) + 1e-10).sqrt()
    return F.avg_pool2d(x * w, size, divisor_override=1) / w.sum()


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


class GeometricMedianWeiszfeld(nn.Module):
    """The geometric median of a map's positions in place of their mean, approximated by ``iterations`` steps of Weiszfeld's algorithm.
    ``intermediate_gradients`` (whether the iterations are part of the autograd graph) is kept and has no meaning in inference."""

    def __init__(self, iterations, intermediate_gradients):
        super().__init__()
        self.iterations = iterations
        self.intermediate_gradients = intermediate_gradients

    def forward(self, x):
        if x.is_cuda:
            from .... import engine
            return engine.geometric_median(_nhwc(x), self.iterations).view(x.size(0), x.size(1), 1, 1)
        return torch.cat([weiszfeld(x[i:i + 1], self.iterations) for i in range(x.size(0))])

    def __repr__(self):
        return "%s(iterations=%s, intermediate_gradients=%s)" % (type(self).__name__, self.iterations, self.intermediate_gradients)


class WeightedGeometricMedianWeiszfeld(nn.Module):
    """The weighted geometric median: a prior weight a_i = ``attention(x)`` per position (w_i = a_i / |m - x_i|).  In the reference's file, not in its POOLINGS."""

    def __init__(self, iterations, intermediate_gradients, attention):
        super().__init__()
        self.iterations = iterations
        self.intermediate_gradients = intermediate_gradients
        self.attention = attention

    def forward(self, x):
        if x.is_cuda:
            from .... import engine
            if not isinstance(self.attention, attention_layers.L2NormAttention):
                raise NotImplementedError("HIP weighted geometric median: attention %r is not an L2NormAttention" % (self.attention,))
            fmap = _nhwc(x)
            prior = engine.pixel_attention(fmap, self.attention.normalize_max)
            return engine.geometric_median(fmap, self.iterations, prior=prior).view(x.size(0), x.size(1), 1, 1)
        return torch.cat([weiszfeld(x[i:i + 1], self.iterations, self.attention(x[i:i + 1]).reshape(x.shape[2:])) for i in range(x.size(0))])

    def __repr__(self):
        return "%s(iterations=%s, intermediate_gradients=%s, attention=%r)" % (type(self).__name__, self.iterations, self.intermediate_gradients, self.attention)


POOLINGS = {
    "GeometricMedianWeiszfeld": GeometricMedianWeiszfeld,
}
