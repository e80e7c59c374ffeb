"""The compound criteria of the GAN scenarios, forward only: mirror of ``L1Loss`` / ``MSELoss`` (mdir/components/optim/criterion/base_losses.py:5-14) and of
``MultiheadLoss``, ``CombinationLoss``, ``LossSet`` and ``CycleLoss`` (compound_losses.py:10-22, 53-108).

``map_losses(pairs)`` is the common evaluator: every pair ``(a, b, kind, sigmoid, weight)`` -- ``b`` a tensor of ``a``'s shape or a number, the constant
target of an adversarial term -- gives the mean of ``|a - b|`` (kind "l1") or ``(a - b)^2`` ("mse") per image (dim 0 of ``a``) and over the pair, and the
call gives ``sum(weight * pair mean)``.  On HIP tensors all pairs of a call run in ONE ``gdt_map_loss`` (gandtr_amd/csrc/map_loss.hip: two launches, terms
and sums in float64 added in an order fixed by the shapes, no atomics -- bit-identical from run to run, a pair's result independent of the other pairs;
nothing returns to the host).  On CPU tensors the same formulas are evaluated in torch, in float64.

``L1Loss`` / ``MSELoss`` are torch's criteria with ``reduction="mean"`` by default; ``MultiheadLoss`` puts all its ``l1`` / ``mse`` heads into one call.
Member criteria are resolved through ``GAN_CRITERIA`` here; ``criterion.CRITERIA`` keeps exactly the two retrieval losses, and the adversarial and
patch-NCE registries are unchanged."""
import ctypes
from collections import namedtuple

import torch

from .... import _hip
from . import adversarial, patchnce
from .adversarial import TotalWithIntermediate

KINDS = {"l1": 0, "mse": 1}

MapLosses = namedtuple("MapLosses", ["per_image", "per_pair", "total"])
MapLosses.__doc__ = """per_image: a list of float64 [N_k] tensors, one per pair; per_pair: float64 [n_pairs], the unweighted means; total: 0-dim float64,
sum_k weight_k * per_pair[k] added in index order"""

MapPair = namedtuple("MapPair", ["a", "b", "kind", "sigmoid", "weight"])
MapPair.__doc__ = """one term of map_losses: maps ``a`` and ``b`` (``b`` a tensor of a's shape or a number), kind "l1" | "mse", ``sigmoid``: applied to a and
to a tensor b before the term, ``weight``: the pair's share of the call's total"""


def _pair(p):
    p = p if isinstance(p, MapPair) else MapPair(*p)
    if p.kind not in KINDS:
        raise NotImplementedError("map criterion %r is not provided by this build (available: %s)" % (p.kind, ", ".join(sorted(KINDS))))
    if not torch.is_tensor(p.a) or p.a.numel() == 0:
        raise ValueError("a map is a non-empty tensor")
    if torch.is_tensor(p.b) and p.b.shape != p.a.shape:
        raise ValueError("maps of shapes %s and %s do not pair (no broadcasting)" % (tuple(p.a.shape), tuple(p.b.shape)))
    return p


def _images(a):
    return a.shape[0] if a.dim() > 1 else 1


def map_losses(pairs):
    """[MapPair | (a, b, kind, sigmoid, weight), ..] -> MapLosses (float64, on the maps' device).  The kernel reads fp32: device maps of another dtype are
    converted to fp32 first (``.float()``), CPU maps are widened to float64"""
    pairs = [_pair(p) for p in pairs]
    if not 1 <= len(pairs) <= _hip.MAP_LOSS_MAX_PAIRS:
        raise ValueError("1 .. %d pairs in one call" % _hip.MAP_LOSS_MAX_PAIRS)
    dev = pairs[0].a.device
    if any(p.a.device != dev or (torch.is_tensor(p.b) and p.b.device != dev) for p in pairs):
        raise ValueError("all maps live on one device")
    if dev.type != "cuda":
        per_image, per_pair = [], []
        with torch.no_grad():
            for p in pairs:
                a = p.a.detach().double().reshape(_images(p.a), -1)
                b = p.b.detach().double().reshape(a.shape) if torch.is_tensor(p.b) else torch.full_like(a, float(p.b))
                if p.sigmoid:
                    a, b = torch.sigmoid(a), torch.sigmoid(b) if torch.is_tensor(p.b) else b
                term = (a - b).abs() if p.kind == "l1" else (a - b) ** 2
                per_image.append(term.mean(dim=1))
                per_pair.append(term.mean())
            total = torch.zeros((), dtype=torch.float64)
            for p, v in zip(pairs, per_pair):
                total = total + float(p.weight) * v
        return MapLosses(per_image, torch.stack(per_pair), total)
    lib = _hip.load()
    with torch.cuda.device(dev):
        keep, table, n_img = [], (_hip.MapLossPair * len(pairs))(), []
        for i, p in enumerate(pairs):
            a = p.a.detach().contiguous().float()
            b = p.b.detach().contiguous().float() if torch.is_tensor(p.b) else None
            keep += [a, b]
            n_img.append(_images(a))
            table[i] = _hip.MapLossPair(a.data_ptr(), None if b is None else b.data_ptr(), 0.0 if b is not None else float(p.b), KINDS[p.kind],
                                        1 if p.sigmoid else 0, n_img[i], a.numel(), float(p.weight))
        nbytes = ctypes.c_size_t()
        _hip.check(lib.gdt_map_loss_workspace_bytes(table, len(pairs), ctypes.byref(nbytes)))
        ws = torch.empty(max(nbytes.value // 8, 1), dtype=torch.float64, device=dev)
        out = torch.empty(sum(n_img) + len(pairs) + 1, dtype=torch.float64, device=dev)
        n = sum(n_img)
        _hip.check(lib.gdt_map_loss(table, len(pairs), out.data_ptr(), out[n:].data_ptr(), out[n + len(pairs):].data_ptr(), ws.data_ptr(), nbytes.value,
                                    torch.cuda.current_stream(dev).cuda_stream))
    return MapLosses(list(out[:n].split(n_img)), out[n:n + len(pairs)], out[n + len(pairs)])


class _MapLoss:
    """torch's L1Loss / MSELoss with the reference's default ``reduction="mean"``; "sum" and "none" as torch has them.  fp32 HIP tensors of one shape run
    ``gdt_map_loss`` and give a 0-dim fp32 tensor; everything else (CPU tensors, other dtypes on the device, broadcasting shapes, "none") runs torch's op and
    keeps torch's dtype"""

    kind = None

    def __init__(self, **kwargs):
        kwargs = {"reduction": "mean", **kwargs}
        self.reduction = kwargs.pop("reduction")
        if self.reduction not in ("mean", "sum", "none"):
            raise ValueError("%s is not a valid value for reduction" % (self.reduction,))
        if kwargs:
            raise NotImplementedError("options %s of the %r criterion are not provided by this build" % (sorted(kwargs), self.kind))

    def _torch(self, input, target):
        fn = torch.nn.functional.l1_loss if self.kind == "l1" else torch.nn.functional.mse_loss
        return fn(input, target, reduction=self.reduction)

    def pairs(self, input, target, weight=1.0, sigmoid=False):
        """this criterion's term of a ``map_losses`` call"""
        return MapPair(input, target, self.kind, sigmoid, weight)

    def evaluate_many(self, pairs):
        """[(input, target), ..] -> float64 [n]: this criterion (reduction "mean" or "sum") on every pair, in one call on the device"""
        if self.reduction == "none":
            raise ValueError("evaluate_many reduces: reduction 'mean' or 'sum'")
        out = map_losses([self.pairs(a, b) for a, b in pairs]).per_pair
        if self.reduction == "sum":
            out = out * torch.tensor([float(a.numel()) for a, _ in pairs], dtype=torch.float64, device=out.device)
        return out

    def forward(self, input, target):
        if not (torch.is_tensor(input) and torch.is_tensor(target)):
            raise ValueError("input and target are tensors")
        if (input.is_cuda and input.dtype == torch.float32 and target.dtype == torch.float32 and self.reduction != "none" and input.shape == target.shape
                and input.numel() > 0):
            return self.evaluate_many([(input, target)])[0].float()
        return self._torch(input, target)

    __call__ = forward

    def to(self, device):
        return self

    def __repr__(self):
        return "%s(reduction=%s)" % (type(self).__name__, self.reduction)


class L1Loss(_MapLoss):
    kind = "l1"


class MSELoss(_MapLoss):
    kind = "mse"


class MultiheadLoss:
    """Combination loss for multi-headed networks, each loss for one head: ``forward(output, target)`` takes two dicts keyed like the losses and returns
    TotalWithIntermediate with ``partial[key] = weights[key] * loss(output[key], target[key])`` and their sum.  ``weights``: a dict with the losses' keys
    (asserted) or one number for all; ``normalize_weights`` divides them by their sum.  On HIP tensors all ``l1`` / ``mse`` heads run in one ``gdt_map_loss``."""

    def __init__(self, weights, normalize_weights, **losses):
        self.losses = {key: initialize_gan_criterion(params) for key, params in losses.items()}
        self.weights = weights
        if isinstance(self.weights, (int, float)):
            self.weights = {key: self.weights for key in self.losses}
        self.weights = dict(self.weights)
        if normalize_weights:
            sum_weights = sum(self.weights.values())
            self.weights = {key: val / sum_weights for key, val in self.weights.items()}
        assert losses.keys() == self.weights.keys(), str(losses.keys()) + "!=" + str(self.weights.keys())
        reductions = [x.reduction for x in self.losses.values()]
        self.reduction = reductions[0] if len(set(reductions)) == 1 else "mixed"

    def _operands(self, key, output, target):
        return output[key], target[key]

    def forward(self, output, target):
        operands = {key: self._operands(key, output, target) for key in self.losses}
        fused = [key for key, crit in self.losses.items() if isinstance(crit, _MapLoss) and crit.reduction != "none" and
                 all(torch.is_tensor(t) and t.is_cuda for t in operands[key]) and operands[key][0].shape == operands[key][1].shape]
        values = {}
        for at in range(0, len(fused), _hip.MAP_LOSS_MAX_PAIRS):
            keys = fused[at:at + _hip.MAP_LOSS_MAX_PAIRS]
            means = map_losses([self.losses[key].pairs(*operands[key], weight=self.weights[key]) for key in keys]).per_pair
            for i, key in enumerate(keys):
                scale = operands[key][0].numel() if self.losses[key].reduction == "sum" else 1
                values[key] = (means[i] * (self.weights[key] * scale)).float()
        total, partial = None, {}
        for key, crit in self.losses.items():
            partial[key] = values[key] if key in values else self.weights[key] * crit(*operands[key])
            total = partial[key] if total is None else total + partial[key]
        return TotalWithIntermediate(total, partial)

    __call__ = forward

    def to(self, device):
        return self

    def __repr__(self):
        return "%s(weights=%s, losses=%s)" % (type(self).__name__, self.weights, self.losses)


class CombinationLoss(MultiheadLoss):
    """Sum of multiple losses on the same data: ``forward(output, target)`` takes one pair of tensors for every loss"""

    def _operands(self, key, output, target):
        return output, target


class LossSet:
    """a bag of criteria under the reference's names (``loss_names``); the epoch iteration picks them"""

    def __init__(self, **losses):
        for key, params in losses.items():
            setattr(self, key, initialize_gan_criterion(params))
        self.reduction = "mixed"
        self.loss_names = set(losses.keys())

    def forward(self, *inputs):
        raise NotImplementedError("Losses are handled manually through epoch iteration")

    __call__ = forward


class CycleLoss:
    """One loss tailored to cycleGAN losses: four member criteria, evaluated by SupervisedCycleGanEpoch"""

    def __init__(self, loss_G_X, loss_G_Y, loss_D_X, loss_D_Y):
        self.loss_G_X = initialize_gan_criterion(loss_G_X)
        self.loss_G_Y = initialize_gan_criterion(loss_G_Y)
        self.loss_D_X = initialize_gan_criterion(loss_D_X)
        self.loss_D_Y = initialize_gan_criterion(loss_D_Y)
        self.reduction = "mixed"

    def forward(self, *inputs):
        raise NotImplementedError("Losses are handled manually through SupervisedCycleGanEpoch")

    __call__ = forward


GAN_CRITERIA = {
    "l1": L1Loss,
    "mse": MSELoss,
    "multihead_loss": MultiheadLoss,
    "combination_loss": CombinationLoss,
    "loss_set": LossSet,
    "cycle_loss": CycleLoss,
    "discriminator_loss": adversarial.DiscriminatorLoss,
    "multilayer_patchnce_loss": patchnce.MultilayerPatchNCELoss,
}


def initialize_gan_criterion(params):
    """``{"loss": <label of GAN_CRITERIA>, ..options}`` -> the criterion; nested criteria are resolved through the same registry (``params`` is not changed)"""
    if not params:
        return None
    params = dict(params)
    kind = params.pop("loss")
    if kind not in GAN_CRITERIA:
        raise NotImplementedError("GAN criterion %r is not provided by this build (available: %s)" % (kind, ", ".join(sorted(GAN_CRITERIA))))
    return GAN_CRITERIA[kind](**params)
