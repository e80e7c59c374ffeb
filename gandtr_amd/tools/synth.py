"""Deterministic weight / input synthesiser.

There is no network on the build or GPU boxes, so benchmarks and parity tests run on random-initialised
weights of the reference architectures.  Everything here is generated with a counter-based NumPy Philox
stream keyed by (seed, crc32(parameter name)), so the build container and the GPU box regenerate
bit-identical tensors without shipping them (never rely on reference-side RNG).

State-dict key names follow the reference modules:
  generator  -- mdir/components/model/network/p2p_networks.py:269-313 (``model.<i>...``)
  embedders  -- torchvision vgg16/resnet101 as sliced by external/cirtorch/networks/imageretrievalnet.py:185-190
                (``features.<i>...``) plus ``pool.p`` (layers/pooling.py:40)
  HED        -- mdir/components/model/network/hed.py:30-45
  RCF        -- mdir/components/model/network/rcf.py:28-66
  U-Net      -- mdir/components/model/network/p2p_networks.py:154-161, :197-230 (``model.model.<i>..``, nested through ``model.1`` / ``model.3``)
  PatchSampleF -- mdir/components/model/network/p2p_networks.py:628-636 (``mlp_<i>.{0,2}...``)
"""
import math
import zlib

import numpy as np
import torch


def _rng(seed, name):
    return np.random.Generator(np.random.Philox(key=[int(seed) & 0xFFFFFFFFFFFFFFFF, zlib.crc32(name.encode())]))


def _normal(seed, name, shape, std=1.0, mean=0.0):
    a = _rng(seed, name).standard_normal(size=shape, dtype=np.float32)
    return torch.from_numpy(a * np.float32(std) + np.float32(mean))


def _uniform(seed, name, shape, lo, hi):
    a = _rng(seed, name).random(size=shape, dtype=np.float32)
    return torch.from_numpy(a * np.float32(hi - lo) + np.float32(lo))


def synth_input(seed, shape, clamp=None, name="input"):
    """Seeded N(0,1) input; generator inputs are clamped to [-1, 1] (mean/std 0.5 normalised images)."""
    x = _normal(seed, name, shape)
    return x.clamp_(-clamp, clamp) if clamp else x


def _conv(sd, seed, name, cout, cin, k, bias, gain=None, transposed=False):
    fan_in = cin * k * k
    std = gain if gain is not None else math.sqrt(2.0 / fan_in)
    shape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
    sd[name + ".weight"] = _normal(seed, name + ".weight", shape, std)
    if bias:
        sd[name + ".bias"] = _normal(seed, name + ".bias", (cout,), 0.1)


def _bn(sd, seed, name, c, gamma_scale=1.0):
    sd[name + ".weight"] = _uniform(seed, name + ".weight", (c,), 0.8, 1.2) * gamma_scale
    sd[name + ".bias"] = _normal(seed, name + ".bias", (c,), 0.1)
    sd[name + ".running_mean"] = _normal(seed, name + ".running_mean", (c,), 0.1)
    sd[name + ".running_var"] = _uniform(seed, name + ".running_var", (c,), 0.8, 1.2)
    sd[name + ".num_batches_tracked"] = torch.tensor(1, dtype=torch.long)


def _blur_filt(c, size):
    """the ``filt`` buffer of a Downsample (size 3: outer([1, 2, 1]) / 16) or an Upsample (size 4: outer([1, 3, 3, 1]) / 16): [c, 1, size, size]"""
    row = torch.tensor([1., 2., 1.] if size == 3 else [1., 3., 3., 1.])
    return (row[:, None] * row[None, :] / 16.0)[None, None].repeat(c, 1, 1, 1)


def generator_state(seed=0, norm="instance", ngf=64, n_blocks=9, in_nc=3, out_nc=3, gain=0.02, no_antialias=True, no_antialias_up=True):
    """ResnetGenerator state dict (p2p_networks.py:269-313).  ``norm='instance'``: N(0, gain) conv weights with
    biases (use_bias, :264-267); ``norm='batch'``: kaiming conv weights, no conv bias, non-trivial BN running
    statistics (last BN of every ResnetBlock scaled by 0.5 so nine residual blocks stay O(1)).  ``no_antialias`` False: CUT's down layers -- the conv
    (stride 1, same weight shape), norm, ReLU and a Downsample whose ``filt`` buffer sits at the next index; ``no_antialias_up`` False: CUT's up layers
    -- an Upsample's ``filt`` buffer, then a Conv2d (weights [cout, cin, 3, 3]) in place of the ConvTranspose2d."""
    sd = {}
    inorm = norm == "instance"
    g = gain if inorm else None

    def norm_at(name, c, scale=1.0):
        if not inorm:
            _bn(sd, seed, name, c, scale)

    _conv(sd, seed, "model.1", ngf, in_nc, 7, inorm, g)
    norm_at("model.2", ngf)
    i, c = 4, ngf
    for _ in range(2):
        _conv(sd, seed, "model.%d" % i, 2 * c, c, 3, inorm, g)
        norm_at("model.%d" % (i + 1), 2 * c)
        i, c = i + 3, 2 * c
        if not no_antialias:
            sd["model.%d.filt" % i] = _blur_filt(c, 3)
            i += 1
    for _ in range(n_blocks):
        p = "model.%d.conv_block." % i
        _conv(sd, seed, p + "1", c, c, 3, inorm, g)
        norm_at(p + "2", c)
        _conv(sd, seed, p + "5", c, c, 3, inorm, g)
        norm_at(p + "6", c, 0.5)
        i += 1
    for _ in range(2):
        if not no_antialias_up:
            sd["model.%d.filt" % i] = _blur_filt(c, 4)
            i += 1
        _conv(sd, seed, "model.%d" % i, c // 2, c, 3, inorm, g, transposed=no_antialias_up)
        norm_at("model.%d" % (i + 1), c // 2)
        i, c = i + 3, c // 2
    _conv(sd, seed, "model.%d" % (i + 1), out_nc, c, 7, True, g)
    return sd


def discriminator_state(seed=0, norm="instance", ndf=64, n_layers=3, in_nc=3, gain=0.02):
    """NLayerDiscriminator state dict (p2p_networks.py:533-563): 4x4 convs at the nn.Sequential indices 0, 2, 5, .., the first and the last with a bias,
    the others with one iff ``norm='instance'``; ``norm='batch'``: non-trivial BN running statistics"""
    sd = {}
    inorm = norm == "instance"
    g = gain if inorm else None
    _conv(sd, seed, "model.0", ndf, in_nc, 4, True, g)
    i, c = 2, ndf
    for n in range(1, n_layers + 1):
        cn = ndf * min(2 ** n, 8)
        _conv(sd, seed, "model.%d" % i, cn, c, 4, inorm, g)
        if not inorm:
            _bn(sd, seed, "model.%d" % (i + 1), cn)
        i, c = i + 3, cn
    _conv(sd, seed, "model.%d" % i, 1, c, 4, True, g)
    return sd


def unet_state(seed=0, norm="instance", ngf=64, num_downs=8, in_nc=3, out_nc=3, gain=0.2, up_gain=1.0, out_gain=1.0):
    """UnetGenerator state dict (p2p_networks.py:132-236).  Level i's nn.Sequential is at ``model.model.`` (outermost; submodule at index 1) or
    ``model.model.1.model.`` + (i - 1) times ``3.model.``; down conv at index 0 (outermost) or 1, up conv at 3 (outermost, innermost) or 5, norms at
    2 / 6 (innermost: 4).  ``norm='instance'``: N(0, gain) conv weights, biases on every conv
    (use_bias); ``norm='batch'``: kaiming-scaled weights (an up conv's fan-in counted as the 4 taps x cin that meet one output pixel, times ``up_gain``), no
    conv bias but on the outermost up conv, non-trivial BatchNorm running statistics and affine parameters.  The outermost up conv (no norm behind it) is
    N(0, out_gain * sqrt(2 / (4 cin))) in both cases, so that the pre-tanh map is O(1)."""
    sd = {}
    inorm = norm == "instance"
    widths = [ngf * min(2 ** i, 8) for i in range(num_downs)]          # inner_nc of level i
    block = lambda i: "model.model." + ("1.model." + "3.model." * (i - 1) if i else "")
    for i in range(num_downs):
        last, outer = i == num_downs - 1, i == 0
        cin_down = in_nc if outer else widths[i - 1]
        cout_up = out_nc if outer else widths[i - 1]
        cin_up = widths[i] if last else 2 * widths[i]
        down, up = block(i) + ("0" if outer else "1"), block(i) + ("3" if outer or last else "5")
        _conv(sd, seed, down, widths[i], cin_down, 4, inorm, gain if inorm else None)
        if outer:
            _conv(sd, seed, up, cout_up, cin_up, 4, True, out_gain * math.sqrt(2.0 / (4 * cin_up)), transposed=True)
        else:
            _conv(sd, seed, up, cout_up, cin_up, 4, inorm, gain if inorm else up_gain * math.sqrt(2.0 / (4 * cin_up)), transposed=True)
        if not inorm and not outer:
            if not last:
                _bn(sd, seed, block(i) + "2", widths[i])
            _bn(sd, seed, block(i) + ("4" if last else "6"), cout_up)
    return sd


def p2p_unet_state(label, seed=0, in_channels=3, out_channels=3, out_gain=1.0, **cfg):
    """State dict of one of the normalisation U-Nets (components/model/network/unet.py: ``label`` and the constructor arguments in ``cfg``), filled along
    the family's own layer list, so its keys are the module's: kaiming-scaled conv weights (a k4 / s2 transposed conv's fan-in counted as the 4 taps x cin that
    meet one output pixel), N(0, 0.1) biases wherever the layer has one, non-trivial BatchNorm statistics and affine parameters.  The last layer is
    N(0, out_gain * sqrt(2 / fan_in)) like the others: behind ReLU / LeakyReLU layers of unit scale that leaves the output map O(1)."""
    from ..components.model.network import unet
    full = unet.family_config(label, in_channels, out_channels, **cfg)
    sd = {}

    def fill(layers, prefix, last_conv):
        for i, item in enumerate(layers):
            name = "%s%d" % (prefix, i)
            if item[0] in ("conv", "convt"):
                _, cin, cout, opts = item
                k = opts.get("kernel_size", 1)
                tr = item[0] == "convt"
                stride = opts.get("stride", 1)
                fan = cin * k * k // (stride * stride) if tr else cin * k * k
                gain = math.sqrt(2.0 / fan) * (out_gain if item is last_conv else 1.0)
                _conv(sd, seed, name, cout, cin, k, opts.get("bias", True), gain, transposed=tr)
            elif item[0] == "bn":
                _bn(sd, seed, name, item[1])
            elif item[0] == "skip":
                fill(item[1], name + ".nested.", last_conv)

    layers = unet.family_layers(label, full)
    fill(layers, "outerblock.", [it for it in layers if it[0] in ("conv", "convt")][-1])
    return sd


def orig_unet_state(seed=0, in_channels=3, out_channels=3, nested_levels=4, min_channels=64, out_gain=1.0):
    """State dict of ``orig_unet`` (components/model/network/unet.py, OrigUNet), keys in the module's order: kaiming-scaled 3x3 conv weights, the
    ConvTranspose2d(k2, s2) counted with the fan-in that meets one output pixel (cin: one tap), N(0, 0.1) biases everywhere; ``outconv`` is
    N(0, out_gain * sqrt(2 / 64)), which leaves the output map O(1) behind ReLU layers of unit scale."""
    sd = {}

    def conv_block(prefix, cin, cout):
        _conv(sd, seed, prefix + "conv1", cout, cin, 3, True)
        _conv(sd, seed, prefix + "conv2", cout, cout, 3, True)

    def block(prefix, level, cin):
        c = min_channels * 2 ** level
        if level == nested_levels:
            conv_block(prefix, cin, c)
            return
        conv_block(prefix + "downconv.", cin, c)
        block(prefix + "nested.", level + 1, c)
        _conv(sd, seed, prefix + "convT", c, 2 * c, 2, True, math.sqrt(2.0 / (2 * c)), transposed=True)
        conv_block(prefix + "upconv.", 2 * c, c)

    block("outerblock.", 0, in_channels)
    _conv(sd, seed, "outconv", out_channels, 64, 1, True, out_gain * math.sqrt(2.0 / 64))
    return sd


def dynint_unet_state(seed=0, in_channels=3, out_channels=3, nested_levels=7, outconv_channels=32, outconv_kernel=3, batchnorm=False, out_gain=1.0):
    """State dict of ``outconv_dynint_unet`` (components/model/network/unet.py, OutconvP2pUNetDynamicInterpolate) with the reference's default conv options,
    keys in the module's order (a block's ``down`` Sequential -- conv, [BatchNorm], LeakyReLU, [the nested block] -- in front of its ``up``): kaiming-scaled conv
    weights, N(0, 0.1) biases, non-trivial BatchNorm statistics and affine parameters; the last conv is N(0, out_gain * sqrt(2 / fan_in))."""
    sd = {}
    widths = ([(64, 128), (128, 256), (256, 512)] + [(512, 512)] * max(0, nested_levels - 3))[:nested_levels]

    def block(prefix, level):
        outer, inter = widths[level]
        last = level + 1 == nested_levels
        _conv(sd, seed, prefix + "down.0", inter, outer, 4, True)
        if batchnorm:
            _bn(sd, seed, prefix + "down.1", inter)
        if not last:
            block("%sdown.%d." % (prefix, 3 if batchnorm else 2), level + 1)
        _conv(sd, seed, prefix + "up.0", outer, inter * (1 if last else 2), 3, True)
        if batchnorm:
            _bn(sd, seed, prefix + "up.1", outer)

    _conv(sd, seed, "down.0", 64, in_channels, 4, True)
    if nested_levels:
        block("down.2.", 0)
    _conv(sd, seed, "up.0", outconv_channels, 128, 3, True)
    k = outconv_kernel
    _conv(sd, seed, "up.2", out_channels, outconv_channels, k, True, out_gain * math.sqrt(2.0 / (outconv_channels * k * k)))
    return sd


def patchsample_state(seed=0, channels=(128, 256, 256, 256), nc=256, gain=1.0):
    """PatchSampleF state dict (p2p_networks.py:628-636): per feature map i of ``channels[i]`` channels ``mlp_<i>.0`` Linear(channels[i], nc) and
    ``mlp_<i>.2`` Linear(nc, nc), N(0, gain * sqrt(2 / fan_in)) weights and N(0, 0.1) biases: on O(1) features the hidden and the output rows are O(1)"""
    sd = {}
    for i, c in enumerate(channels):
        for j, fan_in in ((0, c), (2, nc)):
            name = "mlp_%d.%d" % (i, j)
            sd[name + ".weight"] = _normal(seed, name + ".weight", (nc, fan_in), gain * math.sqrt(2.0 / fan_in))
            sd[name + ".bias"] = _normal(seed, name + ".bias", (nc,), 0.1)
    return sd


def patchnce_maps(seed, shape, mix=0.5):
    """a pair of seeded fp32 feature maps (q side, k side) of ``shape``: the k map is ``mix`` of the q map plus independent noise, so a patch and its
    translation are related (positive logits above the negatives') without being equal -- the row losses spread over a range"""
    q = _normal(seed, "nce.q", shape)
    k = q * np.float32(mix) + _normal(seed, "nce.k", shape) * np.float32(math.sqrt(1.0 - mix * mix))
    return q, k


VGG16_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512]


def vgg16_state(seed=0, p=3.0, width_div=1):
    """GeM-VGG16 embedder state dict: ``features.{0,2,5,...,28}.{weight,bias}`` + ``pool.p``."""
    sd, i, cin = {}, 0, 3
    for v in VGG16_CFG:
        if v == "M":
            i += 1
            continue
        _conv(sd, seed, "features.%d" % i, v // width_div, cin, 3, True)
        cin, i = v // width_div, i + 2
    sd["pool.p"] = torch.ones(1) * p
    return sd


def resnet101_state(seed=0, p=3.0, blocks=(3, 4, 23, 3), width_div=1):
    """GeM-ResNet-101 embedder state dict: ``features.0`` conv1, ``features.1`` bn1, ``features.{4..7}.<b>.*``
    Bottlenecks (bn3 gamma x0.25 so the residual stream stays O(1) without calibrated statistics) + ``pool.p``."""
    sd = {}
    base = 64 // width_div
    _conv(sd, seed, "features.0", base, 3, 7, False)
    _bn(sd, seed, "features.1", base)
    inpl = base
    for li, nb in enumerate(blocks):
        planes = base * (2 ** li)
        for b in range(nb):
            q = "features.%d.%d." % (4 + li, b)
            _conv(sd, seed, q + "conv1", planes, inpl, 1, False)
            _bn(sd, seed, q + "bn1", planes)
            _conv(sd, seed, q + "conv2", planes, planes, 3, False)
            _bn(sd, seed, q + "bn2", planes)
            _conv(sd, seed, q + "conv3", planes * 4, planes, 1, False)
            _bn(sd, seed, q + "bn3", planes * 4, 0.25)
            if b == 0:
                _conv(sd, seed, q + "downsample.0", planes * 4, inpl, 1, False)
                _bn(sd, seed, q + "downsample.1", planes * 4)
            inpl = planes * 4
    sd["pool.p"] = torch.ones(1) * p
    return sd


def resnet_basic_state(seed=0, p=3.0, blocks=(2, 2, 2, 2), width_div=1):
    """GeM-ResNet-18 (blocks (2, 2, 2, 2)) / -34 ((3, 4, 6, 3)) embedder state dict: ``features.0`` conv1, ``features.1`` bn1,
    ``features.{4..7}.<b>.*`` BasicBlocks -- two 3x3 convs, a ``downsample`` only where stride or width change, so not in
    ``features.4.0`` -- (bn2 gamma x0.25 so the residual stream stays O(1) without calibrated statistics) + ``pool.p``."""
    sd = {}
    base = 64 // width_div
    _conv(sd, seed, "features.0", base, 3, 7, False)
    _bn(sd, seed, "features.1", base)
    inpl = base
    for li, nb in enumerate(blocks):
        planes = base * (2 ** li)
        for b in range(nb):
            q = "features.%d.%d." % (4 + li, b)
            _conv(sd, seed, q + "conv1", planes, inpl, 3, False)
            _bn(sd, seed, q + "bn1", planes)
            _conv(sd, seed, q + "conv2", planes, planes, 3, False)
            _bn(sd, seed, q + "bn2", planes, 0.25)
            if b == 0 and (li > 0 or inpl != planes):
                _conv(sd, seed, q + "downsample.0", planes, inpl, 1, False)
                _bn(sd, seed, q + "downsample.1", planes)
            inpl = planes
    sd["pool.p"] = torch.ones(1) * p
    return sd


HED_BLOCKS = ((64, 64), (128, 128), (256, 256, 256), (512, 512, 512), (512, 512, 512))


def hed_state(seed=0, width_div=1):
    """HedInterpolation state dict (hed.py:30-45)."""
    sd, cin = {}, 3
    for bi, chans in enumerate(HED_BLOCKS):
        off = 0 if bi == 0 else 1
        for ci, c in enumerate(chans):
            _conv(sd, seed, "vgg%d.%d" % (bi + 1, off + 2 * ci), c // width_div, cin, 3, True)
            cin = c // width_div
        _conv(sd, seed, "score%d" % (bi + 1), 1, cin, 1, True, gain=1.0 / math.sqrt(cin))
    _conv(sd, seed, "fusion.0", 1, 5, 1, True, gain=0.5)
    return sd


RCF_BLOCKS = ((64, 64), (128, 128), (256, 256, 256), (512, 512, 512), (512, 512, 512))


def rcf_state(seed=0, width_div=1):
    """RCF state dict (rcf.py:28-66): kaiming trunk, and side / score / fuse weights scaled so that on Caffe-range inputs (|x| ~ 100, what the
    rcfngan wrapper chain produces) the pre-sigmoid edge map is O(1-10): the sigmoid is not saturated and still tells results apart."""
    sd, cin = {}, 3
    for bi, chans in enumerate(RCF_BLOCKS):
        for ci, c in enumerate(chans):
            _conv(sd, seed, "conv%d_%d" % (bi + 1, ci + 1), c // width_div, cin, 3, True)
            cin = c // width_div
    for bi, chans in enumerate(RCF_BLOCKS):
        for ci, c in enumerate(chans):
            _conv(sd, seed, "conv%d_%d_down" % (bi + 1, ci + 1), 21, c // width_div, 1, True, gain=0.02 / math.sqrt(c // width_div))
    for bi in range(5):
        _conv(sd, seed, "score_dsn%d" % (bi + 1), 1, 21, 1, True, gain=1.0 / math.sqrt(21))
    _conv(sd, seed, "score_fuse", 1, 5, 1, True, gain=0.5)
    return sd


def whitening_state(seed, dim):
    """Synthetic learned-whitening ``{'P': DxD, 'm': Dx1}`` (format: wrapper.py:315-317, stages/whiten.py:75):
    a well-conditioned random matrix (random diagonal + small dense part; elementwise-deterministic) and a small mean."""
    a = _rng(seed, "lw.P").standard_normal(size=(dim, dim), dtype=np.float32)
    scale = _rng(seed, "lw.s").random(size=(dim,), dtype=np.float32) * np.float32(1.5) + np.float32(0.5)
    P = (a * np.float32(0.3 / math.sqrt(dim)) + np.diag(scale)).astype(np.float32)
    m = (_rng(seed, "lw.m").standard_normal(size=(dim, 1)) * 0.01).astype(np.float32)
    return {"P": P, "m": m}
