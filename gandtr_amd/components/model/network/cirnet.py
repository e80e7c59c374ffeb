"""Retrieval embedder -- host mirror of
  mdir/external/cirtorch/layers/functional.py:11-123 (mac, spoc, gem, rmac, roipool), :130-131 (l2n)
  mdir/external/cirtorch/layers/pooling.py:12-113 (MAC, SPoC, GeM, GeMmp, RMAC, Rpool), layers/normalization.py:10-20 (L2N)
  mdir/external/cirtorch/networks/imageretrievalnet.py:86-123 (ImageRetrievalNet), :146-309 (init_network)
  mdir/components/model/network/cirnet.py:8-65 (CirRetrievalNet, init_cirnet), :68-104 (CirRetrievalNetPreprocessing, init_cirnet_inchan),
  :107-137 (CirRetrievalNetAttention, init_cirnet_attention)
The whole descriptor head runs on the HIP path: any of the five poolings, made regional or not, with the local, the regional
and the final whitening layers (engine.build_embedder, csrc/pool_head.hip); the hub configuration (mdir/hub/embedding.yml:6-10:
plain GeM, no whitening layers) keeps its own two-launch op.  The attention net's weights are computed and folded into the pooling pass there too
(pixel_norm_kernel, the weighted pool_regions_kernel), and the EdgeFilter of the edge-map net is evaluated by the input pack (csrc/aux_kernels.hip).
The dict-valued pooling of init_cirnet (mdir/components/model/network/cirnet.py:61-63), ``{"type": "GeometricMedianWeiszfeld", "iterations": k,
"intermediate_gradients": b}`` (layers/pooling.py), has a head op of its own (engine.HipNet.median_head, csrc/median_pool.hip).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.parameter import Parameter

from . import backbones
from ..layers import attention as attention_layers, pooling as pooling_layers, preprocessing as preprocessing_layers
from ._hipbacked import HipBacked, ScaledInput


def gem(x, p=3, eps=1e-6):
    return F.avg_pool2d(x.clamp(min=eps).pow(p), (x.size(-2), x.size(-1))).pow(1. / p)


def l2n(x, eps=1e-6):
    return x / (torch.norm(x, p=2, dim=1, keepdim=True) + eps).expand_as(x)


def mac(x):
    return F.max_pool2d(x, (x.size(-2), x.size(-1)))


def spoc(x):
    return F.avg_pool2d(x, (x.size(-2), x.size(-1)))


def region_grid(H, W, L=3):
    """The square regions R-MAC lays over an H x W map, as (y0, x0, side) in the order the reference visits them (levels 1..L, rows, columns;
    the whole map is not in the list).  The reference places them with float32 TENSOR arithmetic (functional.py:79-115) and so does this: the
    same expressions in double or integer arithmetic put some regions one pixel off for some map sizes.  csrc/pool_head.hip (gdt_rpool_regions)
    restates it in C for the planner; tests/test_descriptor_heads_host.py holds both to the reference's own grid for every size up to 72 x 72."""
    ovr = 0.4                                           # desired overlap of neighbouring regions
    steps = torch.tensor([2., 3., 4., 5., 6., 7.])      # candidate region counts along the long side
    w = min(W, H)
    b = (max(H, W) - w) / (steps - 1)
    idx = int(torch.min(torch.abs(((w ** 2 - w * b) / w ** 2) - ovr), 0)[1])
    Wd = idx + 1 if H < W else 0                        # extra regions along the longer side
    Hd = idx + 1 if H > W else 0
    out = []
    for l in range(1, L + 1):
        wl = math.floor(2 * w / (l + 1))
        if wl == 0:
            continue
        wl2 = math.floor(wl / 2 - 1)
        bw = 0 if l + Wd == 1 else (W - wl) / (l + Wd - 1)
        bh = 0 if l + Hd == 1 else (H - wl) / (l + Hd - 1)
        xs = (torch.floor(wl2 + torch.arange(l + Wd, dtype=torch.float32) * bw).int() - wl2).tolist()
        ys = (torch.floor(wl2 + torch.arange(l + Hd, dtype=torch.float32) * bh).int() - wl2).tolist()
        out.extend((y, x, wl) for y in ys for x in xs)
    return out


def rmac(x, L=3, eps=1e-6):
    """R-MAC: the l2-normalised maxima of the whole map and of every region, summed (not normalised again)"""
    v = l2n(mac(x), eps)
    for y0, x0, wl in region_grid(x.size(2), x.size(3), L):
        v = v + l2n(mac(x[:, :, y0:y0 + wl, x0:x0 + wl]), eps)
    return v


def roipool(x, rpool, L=3, eps=1e-6):
    """``rpool`` of the whole map and of every region: N x R x D x 1 x 1"""
    vecs = [rpool(x).unsqueeze(1)]
    for y0, x0, wl in region_grid(x.size(2), x.size(3), L):
        vecs.append(rpool(x.narrow(2, y0, wl).narrow(3, x0, wl)).unsqueeze(1))
    return torch.cat(vecs, dim=1)


class MAC(nn.Module):
    def forward(self, x):
        return mac(x)

    def __repr__(self):
        return type(self).__name__ + "()"


class SPoC(nn.Module):
    def forward(self, x):
        return spoc(x)

    def __repr__(self):
        return type(self).__name__ + "()"


class GeM(nn.Module):
    def __init__(self, p=3, eps=1e-6):
        super().__init__()
        self.p = Parameter(torch.ones(1) * p)
        self.eps = eps

    def forward(self, x):
        return gem(x, p=self.p, eps=self.eps)

    def __repr__(self):
        return "%s(p=%.4f, eps=%s)" % (type(self).__name__, self.p.data.tolist()[0], self.eps)


class GeMmp(nn.Module):
    """GeM with one exponent per channel"""

    def __init__(self, p=3, mp=1, eps=1e-6):
        super().__init__()
        self.p = Parameter(torch.ones(mp) * p)
        self.mp = mp
        self.eps = eps

    def forward(self, x):
        return gem(x, p=self.p.unsqueeze(-1).unsqueeze(-1), eps=self.eps)

    def __repr__(self):
        return "%s(p=[%s], eps=%s)" % (type(self).__name__, self.mp, self.eps)


class RMAC(nn.Module):
    def __init__(self, L=3, eps=1e-6):
        super().__init__()
        self.L = L
        self.eps = eps

    def forward(self, x):
        return rmac(x, L=self.L, eps=self.eps)

    def __repr__(self):
        return "%s(L=%s)" % (type(self).__name__, self.L)


class L2N(nn.Module):
    def __init__(self, eps=1e-6):
        super().__init__()
        self.eps = eps

    def forward(self, x):
        return l2n(x, eps=self.eps)

    def __repr__(self):
        return "%s(eps=%s)" % (type(self).__name__, self.eps)


class Rpool(nn.Module):
    """A pooling made regional: ``rpool`` per region, l2n, optional whitening + l2n per region, then sum + l2n over an image's regions"""

    def __init__(self, rpool, whiten=None, L=3, eps=1e-6):
        super().__init__()
        self.rpool = rpool
        self.L = L
        self.whiten = whiten
        self.norm = L2N()
        self.eps = eps

    def forward(self, x, aggregate=True):
        o = roipool(x, self.rpool, self.L, self.eps)             # N x R x D x 1 x 1
        s = o.size()
        o = self.norm(o.view(s[0] * s[1], s[2], s[3], s[4]))
        if self.whiten is not None:
            o = self.norm(self.whiten(o.squeeze(-1).squeeze(-1)))
        o = o.view(s[0], s[1], s[2], s[3], s[4])
        if aggregate:
            o = self.norm(o.sum(1, keepdim=False))              # N x D x 1 x 1
        return o

    def __repr__(self):
        return super().__repr__() + "(L=%s)" % self.L


POOLING = {"mac": MAC, "spoc": SPoC, "gem": GeM, "gemmp": GeMmp, "rmac": RMAC}


OUTPUT_DIM = {"vgg16": 512, "resnet18": 512, "resnet34": 512, "resnet50": 2048, "resnet101": 2048, "resnet152": 2048}


class ImageRetrievalNet(HipBacked, nn.Module):
    """features -> (local whitening) -> pool -> L2N -> (whitening -> L2N); returns D x N (one column per image)."""

    def __init__(self, features, lwhiten, pool, whiten, meta):
        super().__init__()
        self.features = features if isinstance(features, nn.Sequential) else nn.Sequential(*features)
        self.lwhiten = lwhiten
        self.pool = pool
        self.whiten = whiten
        self.norm = L2N()
        self.meta = meta

    def forward(self, x):
        scale = None
        if isinstance(x, ScaledInput):
            x, scale = x.tensor, x.scale
        if self._hip_device().type == "cuda":
            return self._forward_hip(x, scale)
        if scale is not None:
            x = F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=False)
        return self._head(self.features(self._preprocess(x)))

    def _preprocess(self, x):
        """what the torch path applies to the (resized) input in front of the trunk"""
        return x

    def _head(self, o):
        """the torch path behind the trunk's map"""
        if self.lwhiten is not None:
            s = o.size()
            o = self.lwhiten(o.permute(0, 2, 3, 1).contiguous().view(-1, s[1]))
            o = o.view(s[0], s[2], s[3], self.lwhiten.out_features).permute(0, 3, 1, 2)
        o = self.norm(self.pool(o)).squeeze(-1).squeeze(-1)
        if self.whiten is not None:
            o = self.norm(self.whiten(o))
        return o.permute(1, 0)

    HIP_TRUNKS = ("vgg16", "resnet18", "resnet34", "resnet50", "resnet101", "resnet152")

    def _hip_head(self):
        """What engine.build_embedder needs to know about the head beyond the state dict, as a hashable tuple (it is part of the cache key of
        the HIP net, so swapping ``pool`` or a whitening layer rebuilds): (pooling kind, regional, L, eps of the pooling, local whitening, final
        whitening).  None for the hub configuration (plain GeM, no whitening layers), which keeps its own op."""
        pool = self.pool
        if type(pool) is pooling_layers.GeometricMedianWeiszfeld:
            iterations = pool.iterations
            if int(iterations) != iterations or not 0 <= iterations <= 64:
                raise NotImplementedError("HIP embedder: the geometric median takes 0..64 iterations, got %r" % (iterations,))
            return ("geometric_median", int(iterations), self.lwhiten is not None, self.whiten is not None)
        regional = isinstance(pool, Rpool)
        inner = pool.rpool if regional else pool
        kinds = {MAC: "mac", SPoC: "spoc", GeM: "gem", GeMmp: "gemmp", RMAC: "rmac"}
        kind = kinds.get(type(inner))
        if kind is None or (regional and kind == "rmac"):
            raise NotImplementedError("HIP embedder: pooling %r is not one of mac / spoc / gem / gemmp / rmac (regional or not; no regions of "
                                      "R-MAC regions)" % (pool,))
        if kind == "gem" and not regional and self.lwhiten is None and self.whiten is None:
            return None
        L = pool.L if regional else (inner.L if kind == "rmac" else 0)
        return (kind, regional, int(L), float(getattr(inner, "eps", 1e-6)), self.lwhiten is not None, self.whiten is not None)

    def _hip_variant(self):
        """What engine.build_embedder needs beyond the head, as a hashable dict-like tuple of (keyword, value) pairs; part of the cache key as well
        (the input channel count is in the state dict, whose stamp the cache holds)."""
        return ()

    def _hip_embedder(self):
        from .... import engine
        if self.meta.get("architecture") not in self.HIP_TRUNKS:
            raise NotImplementedError("HIP embedder supports vgg16 / resnet18 / resnet34 / resnet50 / resnet101 / resnet152 trunks")
        head = self._hip_head()
        variant = self._hip_variant()
        self._hip_check_inference()
        prec = self._hip_precision()
        in_c = int(self.features[0].weight.shape[1])
        return self._hip_net(("embed", prec, head) + ((in_c,) + variant if variant or in_c != 3 else ()),
                             lambda sd, dev: engine.build_embedder(sd, dev, precision=prec, head=head, **dict(variant)))

    def _forward_hip(self, x, scale):
        net = self._hip_embedder()
        return net.forward(x, scale=scale)[net.out_slot].t()      # N x D storage, D x N view (imageretrievalnet.py:123)

    def forward_many(self, xs):
        """``[self(x) for x in xs]`` with the HIP forwards of the list issued concurrently (engine.HipNet.forward_many): the levels of a
        multi-scale pyramid are independent and each is too small to fill the chip."""
        if self._hip_device().type != "cuda" or len(xs) < 2:
            return [self(x) for x in xs]
        net = self._hip_embedder()
        pairs = [(x.tensor, x.scale) if isinstance(x, ScaledInput) else (x, None) for x in xs]
        return [outs[net.out_slot].t() for outs in net.forward_many(pairs)]

    def meta_repr(self):
        lines = ["  (meta): dict("]
        for k in ("architecture", "local_whitening", "pooling", "regional", "whitening", "outputdim", "mean", "std"):
            lines.append("     %s: %s" % (k, self.meta.get(k)))
        return "\n".join(lines) + "\n  )\n"

    def __repr__(self):
        return super().__repr__()[:-1] + self.meta_repr() + ")"


def init_network(params):
    """cirtorch init_network for the configurations that need no download: a randomly initialised trunk (weights arrive through
    load_state_dict) and the head layers created in the reference's order -- local whitening, pooling, regional whitening, final whitening --
    so that a seeded construction draws the same numbers as the reference's."""
    architecture = params.get("architecture", "resnet101")
    local_whitening = params.get("local_whitening", False)
    pooling = params.get("pooling", "gem")
    regional = params.get("regional", False)
    whitening = params.get("whitening", False)
    mean = params.get("mean", [0.485, 0.456, 0.406])
    std = params.get("std", [0.229, 0.224, 0.225])
    pretrained = params.get("pretrained", True)

    if architecture not in backbones.ARCHITECTURES:
        raise ValueError("Unsupported or unknown architecture: {}!".format(architecture))
    if pretrained:
        raise ValueError("pretrained ImageNet trunks need a download; use pretrained=False and load a checkpoint")
    if isinstance(pooling, dict):
        # The reference builds this pooling in init_cirnet, behind an init_network that skipped it (imageretrievalnet.py:228), with
        # ``params['pooling'].pop("type")``: that empties the caller's dict AND the meta that aliases it of the type, so that a net cannot be rebuilt from its
        # own meta.  Deviation: the dict is copied, the caller's is left alone and ``meta["pooling"]`` keeps its ``type``.
        pooling = dict(pooling)
        kind = pooling.get("type")
        if kind == "HordeCascadedKOrder":
            raise NotImplementedError("dict-valued pooling 'HordeCascadedKOrder' is not mirrored: it returns a list, which ImageRetrievalNet.forward "
                                      "(norm(pool(o))) cannot take in the reference itself")
        if kind not in pooling_layers.POOLINGS:
            raise NotImplementedError("dict-valued pooling of type %r is not mirrored; the dict kinds are %s, the named ones %s"
                                      % (kind, sorted(pooling_layers.POOLINGS), sorted(POOLING)))
        if regional:
            raise NotImplementedError("regional=True with a dict-valued pooling: the reference replaces the Rpool by the bare pooling and its "
                                      "parameter_groups then fails; not mirrored")
    elif pooling not in POOLING:
        raise KeyError(pooling)
    if regional and pooling == "rmac":
        raise NotImplementedError("regional=True with pooling='rmac' (R-MAC regions of R-MAC regions) is not mirrored; no published network uses it")
    net_in = backbones.ARCHITECTURES[architecture](pretrained=False)
    if architecture.startswith("vgg"):
        features = list(net_in.features.children())[:-1]      # drop the last MaxPool
    else:
        features = list(net_in.children())[:-2]               # drop avgpool, fc
    last_convs = [m for f in features[-2:] for m in f.modules() if isinstance(m, nn.Conv2d)]
    dim = last_convs[-1].out_channels

    lwhiten = nn.Linear(dim, dim, bias=True) if local_whitening else None
    if isinstance(pooling, dict):           # (a missing ``iterations`` is the constructor's TypeError, as in the reference; no parameters, nothing drawn)
        pool = pooling_layers.POOLINGS[pooling["type"]](**{k: v for k, v in pooling.items() if k != "type"})
    else:
        pool = POOLING[pooling](mp=dim) if pooling == "gemmp" else POOLING[pooling]()
    if regional:
        pool = Rpool(pool, nn.Linear(dim, dim, bias=True))
    whiten = None
    if whitening:
        whiten = nn.Linear(dim, dim, bias=True)
        if isinstance(whitening, str):          # a learned {P, m} file: W v + b = P (v - m)
            from ....tools.utils import fs_load_pickle
            lw = fs_load_pickle(whitening)
            P, m = torch.tensor(lw["P"]), torch.tensor(lw["m"])
            whiten.load_state_dict({"weight": P, "bias": -torch.mm(P, m).squeeze()})
    meta = {"architecture": architecture, "local_whitening": local_whitening, "pooling": pooling, "regional": regional,
            "whitening": whitening, "mean": mean, "std": std, "outputdim": dim, "out_channels": dim}
    return ImageRetrievalNet(features, lwhiten, pool, whiten, meta)


class CirRetrievalNet(ImageRetrievalNet):
    """cirtorch retrieval net with the optimiser parameter groups of the reference (pool exponent: 10x lr, no weight
    decay; whitening layers at the base rate) and BatchNorm layers frozen in eval mode while training."""

    def parameter_groups(self, optimizer_opts):
        groups = [{"params": self.features.parameters()}]
        if self.meta["local_whitening"]:
            groups.append({"params": self.lwhiten.parameters()})
        if not self.meta["regional"]:
            groups.append({"params": self.pool.parameters(), "lr": optimizer_opts["lr"] * 10, "weight_decay": 0})
        else:                                   # the exponent of the regions' pooling, then the regional whitening at the base rate
            groups.append({"params": self.pool.rpool.parameters(), "lr": optimizer_opts["lr"] * 10, "weight_decay": 0})
            if self.pool.whiten is not None:
                groups.append({"params": self.pool.whiten.parameters()})
        if self.whiten is not None:
            groups.append({"params": self.whiten.parameters()})
        return groups

    def train(self, mode=True):
        res = super().train(mode)
        if mode:
            for m in self.modules():
                if "BatchNorm" in type(m).__name__:
                    m.eval()
        return res


def init_cirnet(**params):
    for key in ("local_whitening", "pooling", "regional", "whitening", "pretrained"):
        if key not in params:
            raise ValueError("Key '%s' not in params" % key)
    params["mean"] = [0.485, 0.456, 0.406]
    params["std"] = [0.229, 0.224, 0.225]
    params["architecture"] = params.pop("cir_architecture")
    net = init_network(params)
    net.meta["in_channels"] = 3
    net.meta["out_channels"] = net.meta["outputdim"]
    return CirRetrievalNet(net.features, net.lwhiten, net.pool, net.whiten, net.meta)


class CirRetrievalNetPreprocessing(CirRetrievalNet):
    """CirRetrievalNet behind a preprocessing layer applied to the net's input (behind whatever the wrappers did: the resize of cirmultiscale,
    meanstd_pre); the layer's parameters train at 10x lr.  On a HIP device the EdgeFilter is part of the input pack."""

    def __init__(self, preprocessing, features, lwhiten, pool, whiten, meta):
        super().__init__(features, lwhiten, pool, whiten, meta)
        self.preprocessing = preprocessing

    def _preprocess(self, x):
        return self.preprocessing(x)

    def _hip_variant(self):
        f = self.preprocessing
        if not isinstance(f, preprocessing_layers.EdgeFilter):
            raise NotImplementedError("HIP embedder: preprocessing %r is not an EdgeFilter" % (f,))
        # (p and tau are parameters: the builder reads them from the state dict, and the cache's stamp sees them change)
        return (("preprocessing", ("edgefilter", f.w, None, f.beta, None, f.eps)),)

    def parameter_groups(self, optimizer_opts):
        return super().parameter_groups(optimizer_opts) + [{"params": self.preprocessing.parameters(), "lr": optimizer_opts["lr"] * 10}]


def init_cirnet_inchan(inputs, **params):
    """init_cirnet for ``inputs["channels"]`` 1 or 3 input channels (1: the first conv's weight summed over its input dimension) behind
    ``inputs["preprocessing"]``: falsy, or {"type": "edgefilter", w, p, beta, tau, eps}"""
    model = init_cirnet(**params)
    if inputs["channels"] == 1:
        first = model.features[0]
        first.in_channels = 1
        first.weight.data = first.weight.data.sum(dim=1, keepdim=True)
        model.meta["in_channels"] = 1
    elif inputs["channels"] != 3:
        raise NotImplementedError("Unsupported number of channels %s" % inputs["channels"])
    if inputs["preprocessing"]:
        model.meta["preprocessing"] = inputs["preprocessing"].pop("type")
        if model.meta["preprocessing"] != "edgefilter":
            raise NotImplementedError("Unsupported preprocessing type '%s'" % model.meta["preprocessing"])
        layer = preprocessing_layers.EdgeFilter(**inputs["preprocessing"])
        model = CirRetrievalNetPreprocessing(layer, model.features, model.lwhiten, model.pool, model.whiten, model.meta)
    return model


class CirRetrievalNetAttention(CirRetrievalNet):
    """CirRetrievalNet whose map is weighted per position by an attention in front of the pooling: norm(pool(features(x) * att)), D x N.

    The reference's forward (its ``squeeze(0)`` and the broadcast ``feats * att``) only works for a batch of one, which is all ``cirfaketuplebatch``
    feeds it.  What is reproduced here, on the torch and on the HIP path, is that batch-of-one behaviour applied to each image separately: the
    attention, and with ``normalize_max`` its maximum, are the image's own, so that a batch equals its images run one by one.  The reference asserts
    in ``forward`` that there is no local and no final whitening; here that is refused at construction.  The attention's parameters (none for
    ``l2norm``, the group is appended all the same) train at 100x lr."""

    def __init__(self, attention, features, lwhiten, pool, whiten, meta):
        assert not lwhiten and not whiten, "the attention net takes no local and no final whitening layer"
        super().__init__(features, lwhiten, pool, whiten, meta)
        self.attention = attention

    def _head(self, o):
        att = torch.stack([self.attention(o[i:i + 1]).reshape(o.shape[2:]) for i in range(o.size(0))])       # N x H x W, each image's own
        return self.norm(self.pool(o * att.unsqueeze(1))).squeeze(-1).squeeze(-1).permute(1, 0)

    def _hip_head(self):
        head = super()._hip_head()
        if head is not None and (head[-2] or head[-1]):                 # (either form of the tuple ends with: local whitening, final whitening)
            raise NotImplementedError("HIP embedder: the attention net takes no local and no final whitening layer")
        return head

    def _hip_variant(self):
        if not isinstance(self.attention, attention_layers.L2NormAttention):
            raise NotImplementedError("HIP embedder: attention %r is not an L2NormAttention" % (self.attention,))
        return (("attention", ("l2norm", bool(self.attention.normalize_max))),)

    def parameter_groups(self, optimizer_opts):
        return super().parameter_groups(optimizer_opts) + [{"params": self.attention.parameters(), "lr": optimizer_opts["lr"] * 100}]


def init_cirnet_attention(attention, **params):
    """init_cirnet with ``attention`` = {"type": "l2norm", "normalize_max": bool} in front of the pooling"""
    model = init_cirnet(**params)
    layer = attention_layers.ATTENTIONS[attention.pop("type")](**attention)
    return CirRetrievalNetAttention(layer, model.features, model.lwhiten, model.pool, model.whiten, model.meta)


# ---- local descriptors (mdir/external/cirtorch/networks/imageretrievalnet.py:396-427) --------------------------------------------------------

def local_forward(net, x, normalize_max=False):
    """(descriptors N x D x h x w, attention N x h x w) of a batch: ``net.norm(net.features(x))`` -- every position's L2-normalised descriptor --
    and the positions' L2NormAttention value sqrt(sum_c x^2 + 1e-10), divided by the image's maximum when ``normalize_max``.  On a HIP device
    both come from one launch behind the trunk (engine.HipNet.local_head); on the CPU from torch ops.  No gradients on the HIP path."""
    if net._hip_device().type == "cuda":
        from .... import engine
        if net.meta.get("architecture") not in net.HIP_TRUNKS:
            raise NotImplementedError("HIP embedder supports vgg16 / resnet18 / resnet34 / resnet50 / resnet101 / resnet152 trunks")
        if net.lwhiten is not None:
            raise NotImplementedError("local descriptors are taken from the trunk's map: no local whitening")
        variant = net._hip_variant()
        net._hip_check_inference()
        prec = net._hip_precision()
        head = ("local", float(net.norm.eps), bool(normalize_max))
        in_c = int(net.features[0].weight.shape[1])
        hip = net._hip_net(("embed", prec, head) + ((in_c,) + variant if variant or in_c != 3 else ()),
                           lambda sd, dev: engine.build_embedder(sd, dev, precision=prec, head=head, **dict(variant)))
        outs = hip.forward(x)
        return outs[hip.out_slot], outs[hip.attention_slot]
    o = net.features(net._preprocess(x))
    att = (o.pow(2).sum(dim=1) + 1e-10).sqrt()
    if normalize_max:
        att = att / att.flatten(1).max(dim=1)[0].view(-1, 1, 1)
    return net.norm(o), att


def extract_ssl(net, input):
    """D x (h w) local descriptors of one image (imageretrievalnet.py:426-427); the tensor stays on the device"""
    return local_forward(net, input)[0].squeeze(0).reshape(net.meta["out_channels"], -1).detach()


def _local_items(images, image_size, transform, bbxs, device):
    if all(torch.is_tensor(im) for im in images):
        return [im.unsqueeze(0) if im.dim() == 3 else im for im in images]
    from ....datasets import ImagesFromList
    data = ImagesFromList(root="", images=images, imsize=image_size, bbxs=bbxs, transform=transform, device=device)
    return [t.unsqueeze(0) for t in data.batch(range(len(data)))]


def _local_batches(net, items, normalize_max=False, max_batch=32):
    """per item (descriptors D x h x w, attention h x w); items of equal size go through the network as one batch, as stages.validate.extract_vectors
    batches them (the trunk and the local head treat every image of a batch on its own)"""
    device = net._hip_device()
    groups, out = {}, [None] * len(items)
    for i, x in enumerate(items):
        groups.setdefault(tuple(x.shape[1:]), []).append(i)
    with torch.no_grad():
        for idx in groups.values():
            for lo in range(0, len(idx), max_batch):
                part = idx[lo:lo + max_batch]
                desc, att = local_forward(net, torch.cat([items[i].to(device) for i in part], 0), normalize_max)
                for j, i in enumerate(part):
                    out[i] = (desc[j], att[j])
    return out


def extract_local_vectors(net, images, image_size, transform, bbxs=None, ms=[1], msp=1, print_freq=10):
    """per image the D x (h w) matrix of ``extract_ssl`` (imageretrievalnet.py:396-424).  ``images``: image tensors (C x H x W or 1 x C x H x W,
    already transformed) or file names, which ``datasets.ImagesFromList`` loads on the device as the reference's loader does.  More than one scale
    raises NotImplementedError, like the reference.  Tensors stay on the device; images of equal size are batched."""
    if len(ms) != 1:
        raise NotImplementedError("multi-scale local descriptors are not implemented (nor in the reference)")
    net.eval()
    items = _local_items(list(images), image_size, transform, bbxs, net._hip_device())
    return [desc.reshape(desc.shape[0], -1) for desc, _ in _local_batches(net, items)]


def extract_local_features(net, images, image_size, transform, scales=(1,), normalize_max=False):
    """per image ([D x h x w per scale], [h x w attention per scale]): the structure ``layers.grouping.Grouping.forward`` consumes.  A scale other
    than 1 resizes the image bilinearly (``F.interpolate(scale_factor=s, align_corners=False)``, as extract_ms does) in front of the network."""
    net.eval()
    items = _local_items(list(images), image_size, transform, None, net._hip_device())
    per_scale = []
    for s in scales:
        scaled = items if s == 1 else [F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=False) for x in items]
        per_scale.append(_local_batches(net, scaled, normalize_max))
    return [([lv[i][0] for lv in per_scale], [lv[i][1] for lv in per_scale]) for i in range(len(items))]
