"""Edge-map preprocessing layers -- host mirror of mdir/components/model/layers/preprocessing.py:9-29.  On a HIP device the filter is evaluated by the
input pack kernel (csrc/aux_kernels.hip, edge_filter) in fp32, in front of the rounding to the activation type."""
import torch
import torch.nn as nn
from torch.nn.parameter import Parameter


class EdgeFilter(nn.Module):
    """w * max(x, eps)^p / (exp(min(-beta * (x - tau), 50)) + 1): a soft threshold at ``tau`` (a step of slope ~ beta * w / 4) times a power law.  ``p`` and
    ``tau`` are learnable; ``forward`` clamps ``tau`` into [0.01, 0.9] and writes the clamp back into the parameter."""

    def __init__(self, w=10, p=0.5, beta=500, tau=0.1, eps=1e-6):
        super().__init__()
        self.w, self.beta, self.eps = float(w), float(beta), float(eps)
        self.p = Parameter(torch.tensor([p], dtype=torch.float32))
        self.tau = Parameter(torch.tensor([tau], dtype=torch.float32))

    TAU_RANGE = (0.01, 0.9)

    def forward(self, x):
        lo, hi = self.TAU_RANGE
        if bool(((self.tau.data < lo) | (self.tau.data > hi)).any()):          # (written only when it moves: the parameter's version is the HIP cache's stamp)
            self.tau.data.clamp_(lo, hi)
        gate = (-self.beta * (x - self.tau)).clamp(max=50.0).exp() + 1          # clipped: exp overflows to inf for small x otherwise
        return (self.w * x.clamp(min=self.eps).pow(self.p)) / gate

    def __repr__(self):
        return "%s(w=%.4f, p=%.4f, beta=%.4f, tau=%.4f, eps=%f)" % (type(self).__name__, self.w, self.p.item(), self.beta, self.tau.item(), self.eps)
