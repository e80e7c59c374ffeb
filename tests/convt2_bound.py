"""Shared by the GPU tests of the transposed-2 route: a float64 reference of one f16 ConvTranspose2d(k2, s2, p0) layer and the derived bound per output element,
in the model of tests/conv_bound.py (whose ``_conv64`` fixes the k3 transposed form).  No test in here.

Kernel size = stride: every output element sums K = cin products (one input pixel through one kernel tap) and the folded shift in fp32, applies the ReLU in fp32
and stores fp16 once.  With the constants and the reasoning of conv_bound.py,

    bound = e + 2^-11 (|ref| + e) + 2^-25,   e = g_K mag,   g_K = K u / (1 - K u),   mag = sum |a| |w| + |shift|.
"""
import torch
import torch.nn.functional as F

import conv_bound as CB


def layer(a, w, shift, relu=False):
    """``a`` the fp16 numbers the layer consumed [N, cin, H, W]; ``w`` [cin, cout, 2, 2] / ``shift`` [cout] from conv_bound.fold(.., transposed=True)"""
    a, w, shift = a.double(), w.double(), shift.double()
    assert tuple(w.shape[2:]) == (2, 2) and w.shape[0] == a.shape[1]
    K = w.shape[0]
    sh = shift[None, :, None, None]
    pre = F.conv_transpose2d(a, w, None, stride=2) + sh
    mag = F.conv_transpose2d(a.abs(), w.abs(), None, stride=2) + sh.abs()
    e = K * CB.U32 / (1 - K * CB.U32) * mag
    ref = F.relu(pre) if relu else pre
    bound = e + CB.U16 * (ref.abs() + e) + CB.SUB16
    return CB.LayerRef(ref, bound, pre, mag, K)
