"""Learnable photometric normalisation nets -- mirror of mdir/components/model/network/unet.py: ``p2p_unet``, ``outconv_unet``, ``inconv_p2p_unet``,
``aligned_p2p_unet``, ``shallow_p2p_unet``, ``orig_unet`` and ``outconv_dynint_unet``.  Image-to-image nets that sit in front of the embedder, at the
embedder's image sizes.

The last two have module trees of their own, at the end of the file: ``orig_unet`` (OrigUNet: pairs of 3x3 convs, MaxPool2d(2) down, ConvTranspose2d(k2, s2)
up; device graph ``engine.build_orig_unet``, the transposed-2 route of gdt_net_conv) and ``outconv_dynint_unet`` (OutconvP2pUNetDynamicInterpolate: an
F.interpolate back to the size each block received + Conv(k3) in place of every transposed conv, so it takes any image size; ``engine.build_dynint_unet``,
gdt_net_resize).  Both are in ``CLASSES`` under their labels; the model registry (``MODEL_LABELS`` in this package's __init__) lists the first five only.
What follows describes the first five.

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


# ---- orig_unet: the classic U-Net (3x3 conv pairs, max-pool down, ConvTranspose2d(k2, s2) up) -- its own module tree, not an ``outerblock`` Sequential

class OrigConvBlock(nn.Module):
    """Conv3x3(p1) + ReLU, twice"""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels, out_channels, 3, padding=1)
        self.relu1 = nn.ReLU()
        self.conv2 = nn.Conv2d(out_channels, out_channels, 3, padding=1)
        self.relu2 = nn.ReLU()

    def forward(self, x):
        return self.relu2(self.conv2(self.relu1(self.conv1(x))))


class OrigSkipConnBlock(nn.Module):
    """``x1 = downconv(x)``; ``x2 = convT(nested(pool(x1)))``; ``upconv(cat([x1, x2], 1))``"""

    def __init__(self, nested, channels, in_channels=None):
        super().__init__()
        self.downconv = OrigConvBlock(channels // 2 if in_channels is None else in_channels, channels)
        self.pool = nn.MaxPool2d(2)
        self.nested = nested
        self.convT = nn.ConvTranspose2d(2 * channels, channels, 2, stride=2)
        self.upconv = OrigConvBlock(2 * channels, channels)

    def forward(self, x):
        x1 = self.downconv(x)
        return self.upconv(torch.cat([x1, self.convT(self.nested(self.pool(x1)))], dim=1))


class OrigUNet(HipBacked, nn.Module):
    """``orig_unet``: ``nested_levels`` skip blocks of ``min_channels * 2**level`` channels around a conv block of ``min_channels * 2**nested_levels``, then
    ``outconv = Conv2d(64, out_channels, 1)``.  The 64 is the reference's own constant: with ``min_channels != 64`` the net constructs and its forward fails at
    ``outconv`` on the CPU, as the reference's does; on a HIP device it is refused before anything is built.  H and W must be multiples of
    ``2**nested_levels`` (the pools halve, the transposed convs double)."""
    hip_default_precision = "f16"
    label = "orig_unet"

    def __init__(self, in_channels, out_channels, nested_levels=4, min_channels=64):
        nn.Module.__init__(self)
        if nested_levels < 1:
            raise ValueError("orig_unet needs at least one skip block, got nested_levels = %s" % (nested_levels,))
        self.meta = {"in_channels": in_channels, "out_channels": out_channels}
        self._cfg = dict(in_channels=in_channels, out_channels=out_channels, nested_levels=nested_levels, min_channels=min_channels)
        block = OrigConvBlock(min_channels * 2 ** (nested_levels - 1), min_channels * 2 ** nested_levels)
        for level in range(nested_levels - 1, 0, -1):
            block = OrigSkipConnBlock(block, min_channels * 2 ** level)
        self.outerblock = OrigSkipConnBlock(block, min_channels, in_channels=in_channels)
        self.outconv = nn.Conv2d(64, out_channels, 1)

    def forward(self, x):
        if self._hip_device().type == "cuda":
            return self._forward_hip(x)
        return self.outconv(self.outerblock(x))

    def _forward_hip(self, x):
        from .... import engine
        cfg = self._cfg
        prec = self._hip_precision()
        if prec not in ("f16", "f16x3"):
            raise NotImplementedError("HIP orig_unet runs in 'f16' or 'f16x3'; %r is a ResnetGenerator mode" % (prec,))
        engine.orig_unet_check(cfg)
        div = 2 ** cfg["nested_levels"]
        if x.dim() != 4 or x.shape[2] % div or x.shape[3] % div:
            raise ValueError("orig_unet with nested_levels = %d needs H and W divisible by %d, got %s: pad the input with the 'reflectpad_divisible:%d' wrapper"
                             % (cfg["nested_levels"], div, tuple(x.shape), div))
        self._hip_check_inference()
        net = self._hip_net(("orig_unet", prec), lambda sd, dev: engine.build_orig_unet(sd, dev, cfg, precision=prec))
        return net.forward(x)[net.out_slot]


CLASSES["orig_unet"] = OrigUNet


# ---- outconv_dynint_unet: the outconv net with a resize + Conv(k3) in place of every transposed conv -- it returns maps of exactly the size it received

class DynIntSkipConnBlock(nn.Module):
    """``cat([x, up(interpolate(down(x), size of x))], 1)``; ``down`` = Conv [BatchNorm] LeakyReLU(0.2) [the nested block], ``up`` = Conv [BatchNorm] [Dropout] ReLU"""

    def __init__(self, nested, outer_channels, inter_channels, conv_opts, upconv_opts, upsample, batchnorm_opts, batchnorm=True, dropout=False):
        super().__init__()
        self.upsample = upsample
        down = [nn.Conv2d(outer_channels, inter_channels, **conv_opts)]
        if batchnorm:
            down.append(nn.BatchNorm2d(inter_channels, **batchnorm_opts))
        down.append(nn.LeakyReLU(0.2))
        if nested is not None:
            down.append(nested)
        self.down = nn.Sequential(*down)
        up = [nn.Conv2d(inter_channels * (2 if nested is not None else 1), outer_channels, **upconv_opts)]
        if batchnorm:
            up.append(nn.BatchNorm2d(outer_channels, **batchnorm_opts))
        if dropout:
            up.append(nn.Dropout(p=dropout))
        up.append(nn.ReLU())
        self.up = nn.Sequential(*up)

    def forward(self, x):
        y = nn.functional.interpolate(self.down(x), size=x.shape[-2:], mode=self.upsample)
        return torch.cat([x, self.up(y)], dim=1)


class OutconvP2pUNetDynamicInterpolate(HipBacked, nn.Module):
    """``outconv_dynint_unet``: Conv(k4, s2, p1) + LeakyReLU(0.2) to 64 channels, ``nested_levels`` skip blocks (64 -> 128 -> 256 -> 512 -> 512 ..), a resize to
    the input's size, Conv(k3) to ``outconv_channels`` + ReLU, a k x k conv.  No transposed conv: every block resizes its result to the size it received, so the
    net takes any H x W whose innermost map is not empty (no ``reflectpad_divisible`` in front)."""
    hip_default_precision = "f16"
    label = "outconv_dynint_unet"

    def __init__(self, in_channels, out_channels, conv_opts=None, upconv_opts=None, nested_levels=7, upsample="bilinear", outconv_channels=32, outconv_kernel=3,
                 dropout=False, batchnorm=False):
        nn.Module.__init__(self)
        assert outconv_kernel % 2 == 1
        self.upsample = upsample
        conv_opts = {"kernel_size": 4, "stride": 2, "padding": 1, **(conv_opts or {})}
        upconv_opts = {"kernel_size": 3, "stride": 1, "padding": 1, **(upconv_opts or {})}
        self.meta = {"in_channels": in_channels, "out_channels": out_channels}
        self._cfg = dict(in_channels=in_channels, out_channels=out_channels, conv_opts=conv_opts, upconv_opts=upconv_opts, nested_levels=nested_levels,
                         upsample=upsample, outconv_channels=outconv_channels, outconv_kernel=outconv_kernel, dropout=dropout, batchnorm=batchnorm)
        widths = ([(64, 128), (128, 256), (256, 512)] + [(512, 512)] * max(0, nested_levels - 3))[:nested_levels]
        inner = None
        for outer, inter in reversed(widths):
            inner = DynIntSkipConnBlock(inner, outer, inter, conv_opts, upconv_opts, upsample, {}, batchnorm=batchnorm, dropout=dropout)
        self.down = nn.Sequential(nn.Conv2d(in_channels, 64, **conv_opts), nn.LeakyReLU(0.2), inner)
        self.up = nn.Sequential(nn.Conv2d(128, outconv_channels, **upconv_opts), nn.ReLU(),
                                nn.Conv2d(outconv_channels, out_channels, outconv_kernel, padding=outconv_kernel // 2))

    def forward(self, x):
        if self._hip_device().type == "cuda":
            return self._forward_hip(x)
        return self.up(nn.functional.interpolate(self.down(x), size=x.shape[-2:], mode=self.upsample))

    def _forward_hip(self, x):
        from .... import engine
        cfg = self._cfg
        if self.training and (cfg["batchnorm"] or cfg["dropout"]):
            raise NotImplementedError("HIP outconv_dynint_unet is inference-only: call .eval() (BatchNorm uses running statistics, Dropout is the identity)")
        prec = self._hip_precision()
        if prec not in ("f16", "f16x3"):
            raise NotImplementedError("HIP outconv_dynint_unet runs in 'f16' or 'f16x3'; %r is a ResnetGenerator mode" % (prec,))
        engine.dynint_unet_check(cfg)
        if x.dim() != 4 or min(x.shape[2:]) >> (cfg["nested_levels"] + 1) < 1:
            raise ValueError("outconv_dynint_unet with nested_levels = %d halves the map %d times: H and W must be at least %d, got %s"
                             % (cfg["nested_levels"], cfg["nested_levels"] + 1, 2 ** (cfg["nested_levels"] + 1), tuple(x.shape)))
        self._hip_check_inference()
        net = self._hip_net(("outconv_dynint_unet", prec), lambda sd, dev: engine.build_dynint_unet(sd, dev, cfg, precision=prec))
        return net.forward(x)[net.out_slot]


CLASSES["outconv_dynint_unet"] = OutconvP2pUNetDynamicInterpolate
