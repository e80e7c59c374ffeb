"""Learnable photometric normalisation nets -- mirror of mdir/components/model/network/unet.py: ``p2p_unet``, ``outconv_unet``, ``inconv_p2p_unet``,
``aligned_p2p_unet`` and ``shallow_p2p_unet`` (``orig_unet`` and ``outconv_dynint_unet`` are not mirrored).  Image-to-image nets that sit in front of the
embedder, at the embedder's image sizes.

Every net is an ``outerblock`` nn.Sequential: a stem, ONE chain of nested skip blocks, a head.  A skip block returns ``cat([x, nested(x)], 1)``; ``nested`` goes
down by a Conv2d(**conv_opts) (k4, s2, p1 by default) to ``inter`` channels, through the next block if there is one, and up again by a
ConvTranspose2d(**conv_opts) to the block's own channel count.  Block widths: 64 -> 128 -> 256 -> 512 -> 512 -> ..  No activation is in place, so the skip half of
a concatenation is exactly what the block received.

The structure is written ONCE, as data: ``family_layers(label, cfg)`` returns the layer list of a net (tuples, nested lists for the skip blocks).  The nn
modules are instantiated from it (so the module tree, and with it every state-dict key -- ``outerblock.0.weight``, ``outerblock.2.nested.0.weight`` .. -- is the
reference's: tests/test_p2p_unet_host.py compares the key lists), ``gandtr_amd.tools.synth.p2p_unet_state`` fills it, and
``gandtr_amd.engine.build_p2p_unet`` walks it to build the device graph.  On a HIP device the forward is inference only.
"""
import torch
import torch.nn as nn

from ._hipbacked import HipBacked

LABELS = ("p2p_unet", "outconv_unet", "inconv_p2p_unet", "aligned_p2p_unet", "shallow_p2p_unet")
_DOWN_UP = {"kernel_size": 4, "stride": 2, "padding": 1}
#: constructor defaults per label, as the reference has them
DEFAULTS = {
    "p2p_unet": dict(dropout=0, conv_opts=None, batchnorm_opts=None, batchnorm=True, nested_levels=7),
    "outconv_unet": dict(conv_opts=None, batchnorm_opts=None, nested_levels=7, outconv_channels=32, outconv_kernel=3, dropout=False, batchnorm=False),
    "inconv_p2p_unet": dict(conv_opts=None, nested_levels=7),
    "aligned_p2p_unet": dict(conv_opts=None, nested_levels=7),
    "shallow_p2p_unet": dict(conv_opts=None, nested_levels=4),
}
_DEFAULT_CONV_OPTS = {label: dict(_DOWN_UP, bias=False) if label == "p2p_unet" else dict(_DOWN_UP) for label in LABELS}


def family_config(label, in_channels, out_channels, **kw):
    """the full configuration of a net: the label's defaults, the caller's arguments, ``conv_opts`` merged over the label's own"""
    if label not in DEFAULTS:
        raise KeyError(label)
    unknown = set(kw) - set(DEFAULTS[label])
    if unknown:
        raise TypeError("%s takes no argument %s" % (label, sorted(unknown)))
    cfg = dict(DEFAULTS[label], **kw)
    cfg.update(in_channels=in_channels, out_channels=out_channels)
    cfg["conv_opts"] = {**_DEFAULT_CONV_OPTS[label], **(cfg["conv_opts"] or {})}
    if "batchnorm_opts" in cfg:
        cfg["batchnorm_opts"] = dict(cfg["batchnorm_opts"] or {})
    if label == "outconv_unet" and cfg["outconv_kernel"] % 2 != 1:
        raise AssertionError("outconv_kernel must be odd")
    if cfg["nested_levels"] < (0 if label == "outconv_unet" else 1):
        raise ValueError("%s needs at least one skip block, got nested_levels = %s" % (label, cfg["nested_levels"]))
    return cfg


def _conv(cin, cout, **opts):
    return ("conv", cin, cout, opts)


def _convt(cin, cout, **opts):
    return ("convt", cin, cout, opts)


def _same(cin, cout, k):
    """a stride-1 Conv2d that keeps the size"""
    return _conv(cin, cout, kernel_size=k, padding=k // 2) if k > 1 else _conv(cin, cout, kernel_size=1)


def _block(nested, outer, inter, conv_opts, batchnorm=False, batchnorm_opts=None, dropout=0, shallow=False):
    """the layers of one skip block's ``nested`` Sequential; ``nested``: the next block's layers or None"""
    bn = lambda c: [("bn", c, dict(batchnorm_opts or {}))] if batchnorm else []
    if shallow:
        layers = [_conv(outer, inter, **conv_opts), ("relu",), _same(inter, inter, 1), ("relu",)]
        if nested is not None:
            layers.append(("skip", nested))
        return layers + [_convt(inter * (2 if nested is not None else 1), outer, **conv_opts), ("relu",), _same(outer, outer, 1), ("relu",)]
    layers = [_conv(outer, inter, **conv_opts)]
    if nested is not None:
        layers += bn(inter) + [("leaky", 0.2), ("skip", nested)]
    else:
        layers += [("relu",)]
    layers += [_convt(inter * (2 if nested is not None else 1), outer, **conv_opts)] + bn(outer)
    if dropout:
        layers += [("dropout", dropout)]
    return layers + [("relu",)]


def family_layers(label, cfg):
    """the layer list of ``outerblock``: ("conv" | "convt", cin, cout, opts), ("bn", c, opts), ("leaky", slope), ("relu",), ("tanh",), ("dropout", p) and
    ("skip", layers) -- a block that returns cat([x, layers(x)], 1)"""
    n, co = cfg["nested_levels"], cfg["conv_opts"]
    cin, cout = cfg["in_channels"], cfg["out_channels"]
    widths = ([(64, 128), (128, 256), (256, 512)] + [(512, 512)] * max(0, n - 3))[:n]
    inner = None
    for level in reversed(range(n)):
        outer, inter = widths[level]
        if label == "p2p_unet":                       # BatchNorm per cfg; Dropout from the fifth block on
            inner = _block(inner, outer, inter, co, cfg["batchnorm"], cfg["batchnorm_opts"], cfg["dropout"] * (level >= 4))
        elif label == "outconv_unet":
            inner = _block(inner, outer, inter, co, cfg["batchnorm"], cfg["batchnorm_opts"], cfg["dropout"])
        elif label == "shallow_p2p_unet":
            inner = _block(inner, outer, inter, co, shallow=True)
        else:
            inner = _block(inner, outer, inter, co)
    skip = [("skip", inner)] if inner is not None else []
    wide = 128 if inner is not None else 64
    if label == "p2p_unet":
        return [_conv(cin, 64, **co), ("leaky", 0.2)] + skip + [_convt(wide, cout, **{**co, "bias": True}), ("tanh",)]
    if label == "outconv_unet":
        oc, ok = cfg["outconv_channels"], cfg["outconv_kernel"]
        return [_conv(cin, 64, **co), ("leaky", 0.2)] + skip + [_convt(wide, oc, **co), ("relu",), _same(oc, cout, ok)]
    if label == "inconv_p2p_unet":
        return [_same(cin, 64, 1), ("leaky", 0.2), _conv(64, 64, **co), ("leaky", 0.2)] + skip + [_convt(wide, cout, **co), ("tanh",)]
    if label == "aligned_p2p_unet":
        return [_same(cin, 64, 3), ("relu",), _same(64, 64, 3), ("relu",)] + skip + [_same(wide, 64, 3), ("relu",), _same(64, 64, 3), ("relu",), _same(64, cout, 3)]
    return ([_conv(cin, 64, **co), ("relu",), _same(64, 64, 1), ("relu",)] + skip +
            [_convt(wide, 64, **co), ("relu",), _same(64, 64, 1), ("relu",), _same(64, cout, 1)])


def size_divisor(label, cfg):
    """H and W must be multiples of this: one factor 2 per stride-2 conv on the way down (the aligned net's outer convs keep the size)"""
    return 2 ** (cfg["nested_levels"] + (0 if label == "aligned_p2p_unet" else 1))


class SkipConnBlock(nn.Module):
    """``cat([x, nested(x)], 1)``"""

    def __init__(self, layers):
        super().__init__()
        self.nested = _sequential(layers)

    def forward(self, x):
        return torch.cat([x, self.nested(x)], dim=1)


def _sequential(layers):
    mods = []
    for item in layers:
        kind = item[0]
        if kind == "conv":
            mods.append(nn.Conv2d(item[1], item[2], **item[3]))
        elif kind == "convt":
            mods.append(nn.ConvTranspose2d(item[1], item[2], **item[3]))
        elif kind == "bn":
            mods.append(nn.BatchNorm2d(item[1], **item[2]))
        elif kind == "leaky":
            mods.append(nn.LeakyReLU(item[1]))
        elif kind == "relu":
            mods.append(nn.ReLU())
        elif kind == "tanh":
            mods.append(nn.Tanh())
        elif kind == "dropout":
            mods.append(nn.Dropout(p=item[1]))
        else:
            mods.append(SkipConnBlock(item[1]))
    return nn.Sequential(*mods)


class _FamilyNet(HipBacked, nn.Module):
    #: single-pass fp16 like the pix2pix U-Net; "f16x3" is the exact mode; the compensated generator modes "f16c" / "f16ch" do not exist here
    hip_default_precision = "f16"
    label = None

    def _init(self, in_channels, out_channels, **kw):
        nn.Module.__init__(self)
        cfg = family_config(self.label, in_channels, out_channels, **kw)
        self.meta = {"in_channels": in_channels, "out_channels": out_channels}
        self._cfg = cfg
        self.outerblock = _sequential(family_layers(self.label, cfg))

    def forward(self, x):
        if self._hip_device().type == "cuda":
            return self._forward_hip(x)
        return self.outerblock(x)

    def _hip_modes(self):
        prec = self._hip_precision()
        if prec not in ("f16", "f16x3"):
            raise NotImplementedError("HIP %s runs in 'f16' or 'f16x3'; %r is a ResnetGenerator mode" % (self.label, prec))
        return prec

    def _forward_hip(self, x):
        from .... import engine
        cfg = self._cfg
        if self.training and (cfg.get("batchnorm") or cfg.get("dropout")):
            raise NotImplementedError("HIP %s is inference-only: call .eval() (BatchNorm uses running statistics, Dropout is the identity)" % self.label)
        prec = self._hip_modes()
        engine.p2p_unet_check(self.label, cfg)
        div = size_divisor(self.label, cfg)
        if x.dim() != 4 or x.shape[2] % div or x.shape[3] % div:
            raise ValueError("%s with nested_levels = %d needs H and W divisible by %d, got %s: pad the input with the 'reflectpad_divisible:%d' wrapper"
                             % (self.label, cfg["nested_levels"], div, tuple(x.shape), div))
        self._hip_check_inference()
        label = self.label
        net = self._hip_net((label, prec), lambda sd, dev: engine.build_p2p_unet(label, sd, dev, cfg, precision=prec))
        return net.forward(x)[net.out_slot]


class P2pUNet(_FamilyNet):
    """``p2p_unet``: Conv(k4, s2) + LeakyReLU(0.2), the blocks (BatchNorm behind every inner conv, Dropout from the fifth block on), ConvTranspose + Tanh"""
    label = "p2p_unet"

    def __init__(self, in_channels, out_channels, dropout=0, conv_opts=None, batchnorm_opts=None, batchnorm=True, nested_levels=7):
        self._init(in_channels, out_channels, dropout=dropout, conv_opts=conv_opts, batchnorm_opts=batchnorm_opts, batchnorm=batchnorm, nested_levels=nested_levels)


class ShallowP2pUNet(_FamilyNet):
    """``shallow_p2p_unet``: every down / up conv followed by ReLU, a 1x1 conv and ReLU; a 1x1 conv last"""
    label = "shallow_p2p_unet"

    def __init__(self, in_channels, out_channels, conv_opts=None, nested_levels=4):
        self._init(in_channels, out_channels, conv_opts=conv_opts, nested_levels=nested_levels)


class OutconvP2pUNet(_FamilyNet):
    """``outconv_unet``: the last ConvTranspose goes to ``outconv_channels`` + ReLU, then a k x k conv; ``nested_levels=0`` has no skip block"""
    label = "outconv_unet"

    def __init__(self, in_channels, out_channels, conv_opts=None, batchnorm_opts=None, nested_levels=7, outconv_channels=32, outconv_kernel=3, dropout=False,
                 batchnorm=False):
        self._init(in_channels, out_channels, conv_opts=conv_opts, batchnorm_opts=batchnorm_opts, nested_levels=nested_levels, outconv_channels=outconv_channels,
                   outconv_kernel=outconv_kernel, dropout=dropout, batchnorm=batchnorm)


class InconvP2pUNet(_FamilyNet):
    """``inconv_p2p_unet``: a 1x1 conv + LeakyReLU in front of the first down conv; ConvTranspose + Tanh last"""
    label = "inconv_p2p_unet"

    def __init__(self, in_channels, out_channels, conv_opts=None, nested_levels=7):
        self._init(in_channels, out_channels, conv_opts=conv_opts, nested_levels=nested_levels)


class AlignedP2pUNet(_FamilyNet):
    """``aligned_p2p_unet``: two 3x3 convs at full resolution on either side of the blocks -- the first behind them reads the 128-channel concatenation --
    and a 3x3 conv last"""
    label = "aligned_p2p_unet"

    def __init__(self, in_channels, out_channels, conv_opts=None, nested_levels=7):
        self._init(in_channels, out_channels, conv_opts=conv_opts, nested_levels=nested_levels)


CLASSES = {c.label: c for c in (P2pUNet, OutconvP2pUNet, InconvP2pUNet, AlignedP2pUNet, ShallowP2pUNet)}
