"""mirror of mdir/components/optim/criterion/__init__.py and cirlosses.py: the criteria a loader-based validation evaluates.

Only the two retrieval losses are provided, under the reference's labels: ``contrastive`` (ContrastiveLoss, cirlosses.py:7-21) and
``triplet`` (TripletLoss, cirlosses.py:51-61), forward only (no gradients).  The formulas are those of
mdir/external/cirtorch/layers/functional.py:141-173, quirks included: the contrastive distance is ``sqrt(sum((a - b + eps)^2))`` with eps
INSIDE the difference and fixed at 1e-6, the triplet loss uses squared distances without eps.

Two forms.  ``criterion(x, label)`` is the reference's: ``x`` D x N descriptors, tuples side by side as (anchor, positive, negatives..),
``label`` the -1 / 1 / 0 vector (a tensor or a list of tensors); it returns the sum over the tuples (``reduction = "sum"``) as a 0-dim
fp32 tensor.  ``criterion.tuple_losses(vecs, tuples)`` is the indexed one: ``vecs`` D x N descriptors of distinct images, ``tuples`` a
[T][S] table of columns of ``vecs`` (column 0 anchor, 1 positive, 2.. negatives; repeats allowed); it returns every tuple's loss.  On a HIP
tensor both run ``gdt_tuple_loss`` (gandtr_amd/csrc/tuple_loss.hip: one launch for all tuples, nothing returns to the host); the label
form builds the table 0..N-1 from the labels.  On a CPU tensor the same formulas are evaluated in torch."""
import ctypes
import warnings
from collections import namedtuple

import torch

from .... import _hip

TupleLosses = namedtuple("TupleLosses", ["loss", "total", "pair_dist"])
TupleLosses.__doc__ = """loss: fp32 [T], one per tuple; total: 0-dim float64, their sum; pair_dist: fp32 [T][S-1] -- contrastive: the distances D,
triplet: the squared distances -- or None"""


def _table(tuples):
    """(int32 [T][S] tensor, where it lives).  A host table (lists, arrays, CPU tensors) is returned on the CPU, a device table as it is."""
    if torch.is_tensor(tuples):
        t = tuples
    else:
        t = torch.as_tensor(tuples)
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 2:
        raise ValueError("the tuple table is [T][S] with T >= 1 and S >= 2 (anchor, positive, negatives..), got %s" % (tuple(t.shape),))
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError("the tuple table holds integer indices, got %s" % t.dtype)
    return t


def _check_indices(t, n_vec):
    lo, hi = int(t.min()), int(t.max())
    if lo < 0 or hi >= n_vec:
        raise ValueError("tuple index outside [0, %d): min %d, max %d" % (n_vec, lo, hi))


def table_from_labels(label, n):
    """The [T][S] table of the reference's label vector over the columns 0..n-1: every tuple is (-1, 1, 0, .., 0), all of one length."""
    if isinstance(label, (list, tuple)):
        label = torch.cat([torch.as_tensor(x).reshape(-1) for x in label])
    lab = torch.as_tensor(label).reshape(-1).cpu().tolist()
    if len(lab) != n:
        raise ValueError("%d labels for %d descriptors" % (len(lab), n))
    nq = sum(1 for v in lab if v == -1)
    if nq == 0 or n % nq:
        raise ValueError("%d descriptors do not split into %d tuples of one length" % (n, nq))
    s = n // nq
    want = [-1, 1] + [0] * (s - 2)
    if s < 2 or any(lab[i * s:(i + 1) * s] != want for i in range(nq)):
        raise ValueError("every tuple must be labelled (-1, 1, 0, ..): anchor, positive, negatives")
    return torch.arange(n, dtype=torch.int32).reshape(nq, s)


def tuple_loss_hip(vecs, tuples, kind, margin, eps, with_pairs=False):
    """``gdt_tuple_loss`` on D x N descriptors on a HIP device.  A host table is checked against N here and uploaded; a table that is
    already on the device is used as it is (its indices are the caller's promise: the kernel clamps nothing).  Enqueued on the current
    stream without a synchronisation."""
    lib = _hip.load()
    if not torch.is_tensor(vecs) or not vecs.is_cuda:
        raise ValueError("tuple_loss_hip needs the descriptors on a HIP device")
    if vecs.dim() != 2:
        raise ValueError("descriptors are D x N, got %s" % (tuple(vecs.shape),))
    v = vecs.t().contiguous().float()                                  # [N][D]
    n_vec, d = v.shape
    t = _table(tuples)
    if not t.is_cuda:
        _check_indices(t, n_vec)
    elif t.device != v.device:
        raise ValueError("table and descriptors on different devices")
    dev = v.device
    t = t.to(torch.int32).to(dev).contiguous()
    n_tuples, s = t.shape
    need = ctypes.c_size_t()
    with torch.cuda.device(dev):
        _hip.check(lib.gdt_tuple_loss_workspace_bytes(n_tuples, s, ctypes.byref(need)))
        ws = torch.empty(max(need.value, 4), dtype=torch.uint8, device=dev)
        loss = torch.empty(n_tuples, dtype=torch.float32, device=dev)
        total = torch.empty((), dtype=torch.float64, device=dev)
        pairs = torch.empty((n_tuples, s - 1), dtype=torch.float32, device=dev) if with_pairs else None
        _hip.check(lib.gdt_tuple_loss(v.data_ptr(), t.data_ptr(), n_vec, d, n_tuples, s, int(kind), float(margin), float(eps),
                                      pairs.data_ptr() if with_pairs else None, loss.data_ptr(), total.data_ptr(), ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream(dev).cuda_stream))
    return TupleLosses(loss, total, pairs)


def tuple_loss_host(vecs, tuples, kind, margin, eps, with_pairs=False):
    """the same formulas in torch on a CPU tensor (functional.py:141-173 per tuple)"""
    if vecs.dim() != 2:
        raise ValueError("descriptors are D x N, got %s" % (tuple(vecs.shape),))
    v = vecs.t().float()
    t = _table(tuples).long()
    _check_indices(t, v.shape[0])
    with torch.no_grad():
        dif = v[t[:, :1]] - v[t[:, 1:]]                                # [T][S-1][D]
        if kind == 0:
            dist = torch.pow(dif + eps, 2).sum(dim=2).sqrt()
            lbl = torch.zeros_like(dist)
            lbl[:, 0] = 1
            terms = 0.5 * lbl * torch.pow(dist, 2) + 0.5 * (1 - lbl) * torch.pow(torch.clamp(margin - dist, min=0), 2)
        else:
            dist = torch.pow(dif, 2).sum(dim=2)
            terms = torch.clamp(dist[:, :1] - dist[:, 1:] + margin, min=0)
        loss = terms.sum(dim=1)
    return TupleLosses(loss, loss.double().sum(), dist if with_pairs else None)


class _TupleCriterion:
    """forward-only criterion over retrieval tuples; ``kind`` / ``eps`` as gdt_tuple_loss takes them"""

    reduction = "sum"
    kind = None
    eps = 0.0

    def __init__(self, margin):
        self.margin = margin

    def tuple_losses(self, vecs, tuples, with_pairs=False):
        """vecs: D x N descriptors, tuples: [T][S] columns of vecs -> TupleLosses(loss [T], total, pair_dist or None)"""
        run = tuple_loss_hip if vecs.is_cuda else tuple_loss_host
        return run(vecs, tuples, self.kind, self.margin, self.eps, with_pairs=with_pairs)

    def __call__(self, x, label):
        return self.forward(x, label)

    def forward(self, x, label):
        return self.tuple_losses(x, table_from_labels(label, x.shape[1])).total.float()

    def __repr__(self):
        return type(self).__name__ + '(' + 'margin=' + '{:.4f}'.format(self.margin) + ')'


class ContrastiveLoss(_TupleCriterion):
    """cirlosses.py:7-21 over functional.py:141-157"""

    kind = 0
    eps = 1e-6

    def __init__(self, margin, eps=None):
        if eps is not None:
            warnings.warn("Parameter 'eps' in ContrastiveLoss is deprecated and will be removed, remove from configuration", DeprecationWarning)
        super().__init__(margin)


class TripletLoss(_TupleCriterion):
    """cirlosses.py:51-61 over functional.py:160-173"""

    kind = 1


CRITERIA = {
    "contrastive": ContrastiveLoss,
    "triplet": TripletLoss,
}


def initialize_criterion(params):
    if not params:
        return None
    kind = params.pop("loss")
    if kind not in CRITERIA:
        raise NotImplementedError("criterion %r is not provided by this build (available: %s)" % (kind, ", ".join(sorted(CRITERIA))))
    return CRITERIA[kind](**params)
