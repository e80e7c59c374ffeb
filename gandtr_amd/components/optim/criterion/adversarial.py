"""The adversarial criterion of the GAN scenarios, forward only: mirror of ``DiscriminatorLoss`` (mdir/components/optim/criterion/compound_losses.py:25-50)
over torch's ``MSELoss`` / ``BCEWithLogitsLoss`` (mdir/components/optim/criterion/__init__.py:6-8, base_losses.py:11-31), and the per-patch / per-image scores
of a PatchGAN logit map.

``patch_scores(logits, kind)`` takes the N logit maps ``[N][1][h][w]`` of an ``NLayerDiscriminator`` and returns, per image and for the batch, the mean
logit, the mean loss against target 0 and the mean loss against target 1.  On a HIP tensor it is ``gdt_patch_score`` (gandtr_amd/csrc/patch_score.hip):
terms and sums in float64, added in a fixed order, no atomics -- bit-identical from run to run; nothing returns to the host.  On a CPU tensor the same
formulas are evaluated in torch.

This module is NOT reached through ``criterion.CRITERIA`` / ``initialize_criterion``: that registry keeps exactly the two retrieval losses a loader-based
validation evaluates.  The adversarial criterion has its own entry, ``initialize_adversarial_criterion(params)``, here."""
import ctypes
from collections import namedtuple

import torch

from .... import _hip

KINDS = {"mse": 0, "bce_with_logits": 1}

PatchScores = namedtuple("PatchScores", ["mean_logit", "loss_target0", "loss_target1", "total"])
PatchScores.__doc__ = """mean_logit, loss_target0, loss_target1: float64 [N], one per logit map; total: float64 [3], the same three means over the batch"""


def _maps(logits):
    if not torch.is_tensor(logits) or logits.dim() != 4 or logits.shape[1] != 1 or logits.numel() == 0:
        raise ValueError("patch logits are [N][1][h][w], got %s" % (tuple(logits.shape) if torch.is_tensor(logits) else type(logits),))
    return logits.reshape(logits.shape[0], -1)


def _kind(kind):
    if kind not in KINDS:
        raise NotImplementedError("adversarial criterion %r is not provided by this build (available: %s)" % (kind, ", ".join(sorted(KINDS))))
    return KINDS[kind]


def patch_scores(logits, kind="mse"):
    """logits [N][1][h][w] -> PatchScores; ``kind``: 'mse' ((x - t)^2) or 'bce_with_logits' (max(x, 0) - x t + log(1 + exp(-|x|)))"""
    k = _kind(kind)
    x = _maps(logits)
    n, hw = x.shape
    if x.is_cuda:
        lib = _hip.load()
        x = x.contiguous().float()
        dev = x.device
        with torch.cuda.device(dev):
            per = torch.empty((n, 3), dtype=torch.float64, device=dev)
            total = torch.empty(3, dtype=torch.float64, device=dev)
            _hip.check(lib.gdt_patch_score(x.data_ptr(), n, hw, k, per.data_ptr(), total.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        return PatchScores(per[:, 0], per[:, 1], per[:, 2], total)
    with torch.no_grad():
        v = x.double()

        def term(t):
            if k == 0:
                return (v - t) ** 2
            return v.clamp(min=0) - v * t + torch.log1p(torch.exp(-v.abs()))

        per = torch.stack([v.mean(dim=1), term(0.0).mean(dim=1), term(1.0).mean(dim=1)], dim=1)
    return PatchScores(per[:, 0], per[:, 1], per[:, 2], per.mean(dim=0))


TotalWithIntermediate = namedtuple("TotalWithIntermediate", ["total", "partial"])
TotalWithIntermediate.__doc__ = """mdir/tools/loss_value.py:35-44 as far as this criterion fills it: ``total`` a 0-dim fp32 tensor, ``partial`` a dict of them"""


class DiscriminatorLoss:
    """aka adversarial loss: ``criterion(output, full_like(output, target))`` with the reference's call form ``forward(output, is_target_real, device)``.

    The quirk is kept: the reference's target is ``int(not is_target_real)`` (compound_losses.py:47-50) -- a REAL target is 0 and a FAKE target is 1.
    A list of outputs (multiscale discriminator) gives the sum of the parts, each reported as ``layer<k>`` counted from the end (:35-42).

    Built with ``DiscriminatorLoss(criterion={"loss": "mse"})`` or through ``initialize_adversarial_criterion``; it is not an entry of ``criterion.CRITERIA``
    and is not reached through ``initialize_criterion`` (see the module docstring)."""

    reduction = "mixed"

    def __init__(self, criterion=None):
        criterion = dict(criterion or {"loss": "mse"})
        self.kind = criterion.pop("loss")
        _kind(self.kind)
        if criterion:
            raise NotImplementedError("options %s of the %r criterion are not provided by this build" % (sorted(criterion), self.kind))

    @staticmethod
    def get_target(is_target_real):
        return int(not is_target_real)

    def _one(self, output, is_target_real):
        total = patch_scores(output, self.kind).total
        return total[1 + self.get_target(is_target_real)].float()

    def forward(self, output, is_target_real, device=None):
        if isinstance(output, list):
            partial, total = {}, None
            for i, y in enumerate(output):
                key = "layer" + str(len(output) - 1 - i)
                partial[key] = self._one(y, is_target_real)
                total = partial[key] if total is None else total + partial[key]
            return TotalWithIntermediate(total, partial)
        return TotalWithIntermediate(self._one(output, is_target_real), {})

    __call__ = forward

    def __repr__(self):
        return "%s(criterion=%s)" % (type(self).__name__, self.kind)


ADVERSARIAL_CRITERIA = {"discriminator_loss": DiscriminatorLoss}


def initialize_adversarial_criterion(params):
    """``{"loss": "discriminator_loss", "criterion": {"loss": "mse"}}`` -> DiscriminatorLoss.  The adversarial criteria live in this registry alone:
    ``criterion.initialize_criterion`` / ``criterion.CRITERIA`` keep the two retrieval losses and do not know them."""
    if not params:
        return None
    params = dict(params)
    kind = params.pop("loss")
    if kind not in ADVERSARIAL_CRITERIA:
        raise NotImplementedError("adversarial criterion %r is not provided by this build (available: %s)" % (kind, ", ".join(sorted(ADVERSARIAL_CRITERIA))))
    return ADVERSARIAL_CRITERIA[kind](**params)
