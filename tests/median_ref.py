"""Float64 restatement of the geometric-median pooling (csrc/median_pool.hip, layers/pooling.py), per image.  Contains no reference code.

    y_i = s_i x_i,  w_i = a_i;   T times: m = sum_i w_i y_i / sum_i w_i,  w_i = a_i / sqrt(sum_c (y_ic - m_c)^2 + 1e-10);   m = sum_i w_i y_i / sum_i w_i
"""
import torch


def geometric_median(x, iterations, scale=None, prior=None):
    """x: N x H x W x D (NHWC, any float type); scale, prior: N x H x W or None (ones).  Returns float64 N x D; every image on its own."""
    x = x.detach().cpu().double()
    n, h, w, d = x.shape
    y = x.reshape(n, h * w, d)
    if scale is not None:
        y = y * scale.detach().cpu().double().reshape(n, h * w, 1)
    a = prior.detach().cpu().double().reshape(n, h * w) if prior is not None else torch.ones((n, h * w), dtype=torch.float64)
    out = []
    for k in range(n):
        wts = a[k]
        for _ in range(iterations):
            m = (wts[:, None] * y[k]).sum(0) / wts.sum()
            wts = a[k] / ((y[k] - m).pow(2).sum(1) + 1e-10).sqrt()
        out.append((wts[:, None] * y[k]).sum(0) / wts.sum())
    return torch.stack(out)


def nchw(x, iterations, scale=None, prior=None):
    """the same on an N x D x H x W map"""
    return geometric_median(x.permute(0, 2, 3, 1), iterations, scale, prior)
