"""CUT's ``nce`` criterion, forward only: mirror of ``PatchNCELoss`` / ``MultilayerPatchNCELoss`` (mdir/components/optim/criterion/compound_losses.py:113-173)
and of the forward of ``SupervisedCutEpoch.calculate_nce_loss`` (mdir/learning/epoch_iteration/cut_epochs.py:79-89).

For row i of a group of n pooled patch rows: ``out_0 = q_i . k_i / T``, ``out_{1+j} = q_i . k_j / T`` over the n rows of the group with the entry j == i
replaced by ``-10 / T``, ``loss_i = logsumexp(out) - out_0`` (cross entropy against class 0).  ``batch_dim_for_bmm`` is the number of groups: 1 mines the
negatives from the whole batch, the batch size from the image's own patches.

On HIP tensors every layer runs in ONE call of ``gdt_patchnce_loss`` (gandtr_amd/csrc/patch_nce.hip: the [n][n] logits are never written, the layer means
and the total are added in float64 in a fixed order, no atomics -- bit-identical from run to run; nothing returns to the host).  On CPU tensors the
reference's torch ops run.

Like the adversarial criterion this module is NOT reached through ``criterion.CRITERIA`` / ``initialize_criterion``: that registry keeps exactly the two
retrieval losses.  Its entry is ``initialize_patchnce_criterion(params)``, here."""
import torch

from .... import _hip
from .adversarial import TotalWithIntermediate


def _rows(feat_q, feat_k, groups):
    if not (torch.is_tensor(feat_q) and torch.is_tensor(feat_k)) or feat_q.dim() != 2 or feat_q.shape != feat_k.shape or feat_q.numel() == 0:
        raise ValueError("pooled features are two [rows][d] tensors of one shape")
    if groups < 1 or feat_q.shape[0] % groups:
        raise ValueError("%d rows do not split into batch_dim_for_bmm = %d groups" % (feat_q.shape[0], groups))


def patchnce_rows(feat_q_pool, feat_k_pool, batch_dim_for_bmm=1, temperature=0.07, weight=1.0):
    """the layers' pooled rows (lists of [rows][d] HIP tensors) -> (list of fp32 row losses [rows], float64 [L + 1]: mean(row loss * weight) per layer,
    then their sum / L).  Two launches for all layers."""
    if len(feat_q_pool) != len(feat_k_pool) or not 1 <= len(feat_q_pool) <= _hip.PATCH_MAX_LAYERS:
        raise ValueError("1 .. %d layers of q and as many of k" % _hip.PATCH_MAX_LAYERS)
    lib = _hip.load()
    dev = feat_q_pool[0].device
    with torch.cuda.device(dev):
        qs = [q.detach().contiguous().float() for q in feat_q_pool]
        ks = [k.detach().contiguous().float() for k in feat_k_pool]
        table, losses = (_hip.PatchNceLayer * len(qs))(), []
        for i, (q, k) in enumerate(zip(qs, ks)):
            _rows(q, k, batch_dim_for_bmm)
            if k.device != dev or q.device != dev:
                raise ValueError("all pooled features live on one device")
            losses.append(torch.empty(q.shape[0], dtype=torch.float32, device=dev))
            table[i] = _hip.PatchNceLayer(q.data_ptr(), k.data_ptr(), losses[i].data_ptr(), q.shape[0], q.shape[1], int(batch_dim_for_bmm))
        totals = torch.empty(len(qs) + 1, dtype=torch.float64, device=dev)
        _hip.check(lib.gdt_patchnce_loss(table, len(qs), 1.0 / float(temperature), float(weight), totals.data_ptr(),
                                         torch.cuda.current_stream(dev).cuda_stream))
    return losses, totals


class PatchNCELoss:
    """``forward(feat_q, feat_k)`` -> the per-row losses [rows] (the reference's ``CrossEntropyLoss(reduction='none')`` over ``cat(l_pos, l_neg) / T``)"""

    reduction = "mixed"

    def __init__(self, batch_dim_for_bmm=1, temperature=0.07):
        self.mask_dtype = torch.bool
        self.batch_dim_for_bmm = batch_dim_for_bmm
        self.temperature = temperature

    def forward(self, feat_q, feat_k):
        _rows(feat_q, feat_k, self.batch_dim_for_bmm)
        if feat_q.is_cuda:
            return patchnce_rows([feat_q], [feat_k], self.batch_dim_for_bmm, self.temperature)[0][0]
        num_patches, dim = feat_q.shape
        feat_k = feat_k.detach()
        l_pos = torch.bmm(feat_q.view(num_patches, 1, -1), feat_k.view(num_patches, -1, 1)).view(num_patches, 1)
        feat_q = feat_q.view(self.batch_dim_for_bmm, -1, dim)
        feat_k = feat_k.view(self.batch_dim_for_bmm, -1, dim)
        npatches = feat_q.size(1)
        l_neg_curbatch = torch.bmm(feat_q, feat_k.transpose(2, 1))
        diagonal = torch.eye(npatches, device=feat_q.device, dtype=self.mask_dtype)[None, :, :]
        l_neg_curbatch.masked_fill_(diagonal, -10.0)
        out = torch.cat((l_pos, l_neg_curbatch.view(-1, npatches)), dim=1) / self.temperature
        return torch.nn.functional.cross_entropy(out, torch.zeros(out.size(0), dtype=torch.long, device=feat_q.device), reduction="none")

    __call__ = forward

    def __repr__(self):
        return "%s(batch_dim_for_bmm=%s, temperature=%s)" % (type(self).__name__, self.batch_dim_for_bmm, self.temperature)


class MultilayerPatchNCELoss:
    """``forward(feat_q_pool, feat_k_pool)`` -> TotalWithIntermediate: ``partial["layer<k>"] = mean(row loss * weight)`` per nce layer k, ``total`` their sum
    over the number of nce layers.  ``row_losses`` keeps the per-row losses of the last call (a list of [rows] tensors on the features' device)."""

    reduction = "mixed"

    def __init__(self, batch_dim_for_bmm, nce_layers, num_patches, temperature, weight):
        self.nce_layers = [int(i) for i in nce_layers.split(",")] if isinstance(nce_layers, str) else [int(i) for i in nce_layers]
        if not self.nce_layers:
            raise ValueError("nce_layers names at least one layer")
        self.losses = [PatchNCELoss(batch_dim_for_bmm, temperature) for _ in self.nce_layers]
        self.batch_dim_for_bmm = batch_dim_for_bmm
        self.temperature = temperature
        self.num_patches = num_patches
        self.weight = weight
        self.row_losses = None

    def forward(self, feat_q_pool, feat_k_pool):
        n = min(len(feat_q_pool), len(feat_k_pool), len(self.nce_layers))              # the reference zips
        keys = ["layer" + str(layer) for layer in self.nce_layers[:n]]
        if n and feat_q_pool[0].is_cuda:
            rows, totals = patchnce_rows(feat_q_pool[:n], feat_k_pool[:n], self.batch_dim_for_bmm, self.temperature, self.weight)
            self.row_losses = rows
            partial = {key: totals[i].float() for i, key in enumerate(keys)}
            total = totals[n].float() if n == len(self.nce_layers) else (totals[:n].sum() / len(self.nce_layers)).float()
            return TotalWithIntermediate(total, partial)
        total, partial, self.row_losses = torch.zeros(()), {}, []
        for feat_q, feat_k, criterion, key in zip(feat_q_pool, feat_k_pool, self.losses, keys):
            self.row_losses.append(criterion(feat_q, feat_k))
            partial[key] = torch.mean(self.row_losses[-1] * self.weight)
            total = total + partial[key]
        return TotalWithIntermediate(total / len(self.nce_layers), partial)

    __call__ = forward

    def __repr__(self):
        return "%s(batch_dim_for_bmm=%s, nce_layers=%s, num_patches=%s, temperature=%s, weight=%s)" % (
            type(self).__name__, self.batch_dim_for_bmm, self.nce_layers, self.num_patches, self.temperature, self.weight)


PATCHNCE_CRITERIA = {"multilayer_patchnce_loss": MultilayerPatchNCELoss}


def initialize_patchnce_criterion(params):
    """``{"loss": "multilayer_patchnce_loss", "batch_dim_for_bmm": 1, "nce_layers": "4,8,12,16", "num_patches": 256, "temperature": 0.07, "weight": 1.0}``
    -> MultilayerPatchNCELoss.  These criteria live in this registry alone: ``criterion.CRITERIA`` keeps the two retrieval losses and does not know them."""
    if not params:
        return None
    params = dict(params)
    kind = params.pop("loss")
    if kind not in PATCHNCE_CRITERIA:
        raise NotImplementedError("patch-NCE criterion %r is not provided by this build (available: %s)" % (kind, ", ".join(sorted(PATCHNCE_CRITERIA))))
    return PATCHNCE_CRITERIA[kind](**params)


def calculate_nce_loss(criterion, netG, netF, output, target, patch_ids=None):
    """The patch-wise contrastive loss between an image batch ``target`` (q) and its translation ``output`` (k) -- cut_epochs.py:79-89: both go through
    ``netG``'s encoder (``layers=criterion.nce_layers, encode_only=True``), the positions are drawn for k (or taken from ``patch_ids``) and reused for q,
    both are pooled by ``netF`` and scored by ``criterion``.  On a HIP device ``target`` and ``output`` run through the encoder as ONE concatenated batch
    (InstanceNorm and eval-mode BatchNorm act per image) and through ``netF`` in one launch; the result stays on the device."""
    layers = list(criterion.nce_layers)
    if output.is_cuda:
        if output.shape != target.shape:
            raise ValueError("output %s and target %s differ in shape" % (tuple(output.shape), tuple(target.shape)))
        feats = netG.forward(torch.cat([target, output], dim=0), layers=layers, encode_only=True)
        pooled, _ = netF(feats, num_patches=criterion.num_patches, patch_ids=patch_ids)
        half = [p.shape[0] // 2 for p in pooled]
        return criterion([p[:h] for p, h in zip(pooled, half)], [p[h:] for p, h in zip(pooled, half)])
    feat_q = netG.forward(target, layers=list(layers), encode_only=True)
    feat_k = netG.forward(output, layers=list(layers), encode_only=True)
    feat_k_pool, sample_ids = netF(feat_k, num_patches=criterion.num_patches, patch_ids=patch_ids)
    feat_q_pool, _ = netF(feat_q, num_patches=criterion.num_patches, patch_ids=sample_ids)
    return criterion(feat_q_pool, feat_k_pool)
