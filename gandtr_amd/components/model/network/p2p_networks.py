"""CycleGAN / HED-N-GAN ResNet generator, pix2pix U-Net generator, PatchGAN discriminator and CUT's patch sampler -- host mirror of
mdir/components/model/network/p2p_networks.py (get_norm_layer :23-35, UnetGenerator / UnetSkipConnectionBlock :132-236, ResnetGenerator :239-337, ResnetBlock :454-506, NLayerDiscriminator :509-571, Normalize / PatchSampleF :595-671).

The nn.Module tree is identical to the reference's (same nn.Sequential indices, same parameter names, same creation
order), so reference checkpoints load unchanged and seeded initialisation reproduces the reference's weights.  On a
cuda (HIP) device the forward runs on the hand-written kernels through gandtr_amd.engine; on 'cpu' it runs the stock
torch modules (BASELINE config 0: "plumbing, no GPU").
"""
import functools

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ._hipbacked import HipBacked


def get_norm_layer(norm_type="instance", track_running_stats=True):
    """'batch' -> BatchNorm2d(affine, running stats); 'instance' -> InstanceNorm2d(affine=False); 'none' -> identity."""
    if not isinstance(norm_type, str):
        return norm_type
    if norm_type == "batch":
        return functools.partial(nn.BatchNorm2d, affine=True, track_running_stats=track_running_stats)
    if norm_type == "instance":
        return functools.partial(nn.InstanceNorm2d, affine=False)
    if norm_type == "none":
        return lambda _channels: nn.Identity()
    raise NotImplementedError('normalization layer [%s] is not found' % norm_type)


def _pad_layer(padding_type):
    """-> (list of explicit padding modules, conv padding) for a 3x3 conv"""
    if padding_type == "reflect":
        return [nn.ReflectionPad2d(1)], 0
    if padding_type == "replicate":
        return [nn.ReplicationPad2d(1)], 0
    if padding_type == "zero":
        return [], 1
    raise NotImplementedError('padding [%s] is not implemented' % padding_type)


class ResnetBlock(nn.Module):
    """x + norm(conv3x3(pad(relu(norm(conv3x3(pad(x)))))));  sub-module indices 0 pad, 1 conv, 2 norm, 3 relu, 4 pad,
    5 conv, 6 norm (dropout, when enabled, shifts the second half by one -- as in the reference)."""

    def __init__(self, dim, padding_type, norm_layer, use_dropout, use_bias):
        super().__init__()
        layers = []
        pads, p = _pad_layer(padding_type)
        layers += pads + [nn.Conv2d(dim, dim, kernel_size=3, padding=p, bias=use_bias), norm_layer(dim), nn.ReLU(True)]
        if use_dropout:
            layers.append(nn.Dropout(0.5))
        pads, p = _pad_layer(padding_type)
        layers += pads + [nn.Conv2d(dim, dim, kernel_size=3, padding=p, bias=use_bias), norm_layer(dim)]
        self.conv_block = nn.Sequential(*layers)

    def forward(self, x):
        return x + self.conv_block(x)


def _binomial_filter(size):
    """the normalised outer product of the binomial row of ``size`` taps: [1, 2, 1] (3) or [1, 3, 3, 1] (4)"""
    row = torch.tensor({3: [1., 2., 1.], 4: [1., 3., 3., 1.]}[size])
    filt = row[:, None] * row[None, :]
    return filt / filt.sum()


class Downsample(nn.Module):
    """CUT's anti-aliased down-sampling: reflection pad by 1, then a depthwise 3x3 conv at stride 2 with the weights outer([1, 2, 1], [1, 2, 1]) / 16;
    ceil(H / 2) x ceil(W / 2), H and W at least 2.  ``filt`` is a buffer [C, 1, 3, 3], as in the reference's state dicts.  On the HIP path:
    gdt_net_blur_resample, mode 0."""

    def __init__(self, channels):
        super().__init__()
        self.channels = channels
        self.register_buffer("filt", _binomial_filter(3)[None, None].repeat(channels, 1, 1, 1))

    def forward(self, x):
        return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), self.filt, stride=2, groups=x.shape[1])


class Upsample(nn.Module):
    """CUT's anti-aliased up-sampling: replicate pad by 1, a depthwise transposed 4x4 conv at stride 2 with the weights outer([1, 3, 3, 1], [1, 3, 3, 1]) / 16
    and a crop to 2H x 2W -- the function F.interpolate(scale_factor=2, mode="bilinear", align_corners=False) computes.  ``filt`` is a buffer
    [C, 1, 4, 4], as in the reference's state dicts.  On the HIP path: gdt_net_blur_resample, mode 1."""

    def __init__(self, channels):
        super().__init__()
        self.channels = channels
        self.register_buffer("filt", (_binomial_filter(4) * 4)[None, None].repeat(channels, 1, 1, 1))

    def forward(self, x):
        y = F.conv_transpose2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), self.filt, stride=2, padding=2, groups=x.shape[1])
        return y[:, :, 1:-1, 1:-1]


class ResnetGenerator(HipBacked, nn.Module):
    """ResNet generator: 7x7 stem, two down layers, n_blocks ResnetBlocks, two up layers, 7x7 head + tanh.  A down layer is a stride-2 conv
    (``no_antialias``, the hub configuration) or a stride-1 conv + norm + ReLU + Downsample (CUT's default); an up layer is a ConvTranspose
    (``no_antialias_up``) or Upsample + stride-1 conv + norm + ReLU.  Reflect padding without dropout is on the HIP hot path, in all four combinations
    of the two flags; other configurations are rejected with NotImplementedError on a cuda device."""

    #: the generators meet north_star's 1e-3 in the compensated mode only
    hip_default_precision = "f16c"
    #: ``forward(.., encode_only=True)`` on the HIP path runs a graph that ends at the last requested tap; False: the full graph, later layers discarded
    hip_encoder_graph = True

    def __init__(self, input_nc, output_nc, ngf=64, norm_layer="batch", use_dropout=False, n_blocks=9,
                 padding_type="reflect", no_antialias=True, no_antialias_up=True, track_running_stats=True):
        assert n_blocks >= 0
        super().__init__()
        self.meta = {"in_channels": input_nc, "out_channels": output_nc}
        self._cfg = dict(norm=norm_layer if isinstance(norm_layer, str) else None, n_blocks=n_blocks,
                         padding_type=padding_type, use_dropout=use_dropout, no_antialias=no_antialias, no_antialias_up=no_antialias_up)
        norm_layer = get_norm_layer(norm_layer, track_running_stats)
        base = norm_layer.func if isinstance(norm_layer, functools.partial) else norm_layer
        use_bias = base == nn.InstanceNorm2d

        seq = [nn.ReflectionPad2d(3), nn.Conv2d(input_nc, ngf, kernel_size=7, padding=0, bias=use_bias), norm_layer(ngf),
               nn.ReLU(True)]
        ch = ngf
        for _ in range(2):
            seq += [nn.Conv2d(ch, ch * 2, kernel_size=3, stride=2 if no_antialias else 1, padding=1, bias=use_bias), norm_layer(ch * 2), nn.ReLU(True)]
            if not no_antialias:
                seq.append(Downsample(ch * 2))
            ch *= 2
        for _ in range(n_blocks):
            seq.append(ResnetBlock(ch, padding_type=padding_type, norm_layer=norm_layer, use_dropout=use_dropout,
                                   use_bias=use_bias))
        for _ in range(2):
            if no_antialias_up:
                seq += [nn.ConvTranspose2d(ch, ch // 2, kernel_size=3, stride=2, padding=1, output_padding=1, bias=use_bias)]
            else:
                seq += [Upsample(ch), nn.Conv2d(ch, ch // 2, kernel_size=3, stride=1, padding=1, bias=use_bias)]
            seq += [norm_layer(ch // 2), nn.ReLU(True)]
            ch //= 2
        seq += [nn.ReflectionPad2d(3), nn.Conv2d(ngf, output_nc, kernel_size=7, padding=0), nn.Tanh()]
        self.model = nn.Sequential(*seq)

    # ------------------------------------------------------------------------------------------------ forward
    def forward(self, input, layers=[], encode_only=False):
        if self._hip_device().type == "cuda":
            return self._forward_hip(input, list(layers), encode_only)
        if -1 in layers:
            layers.append(len(self.model))
        if len(layers) > 0:
            feat, feats = input, []
            for layer_id, layer in enumerate(self.model):
                feat = layer(feat)
                if layer_id in layers:
                    feats.append(feat)
                if layer_id == layers[-1] and encode_only:
                    return feats
            return feat, feats
        return self.model(input)

    def _forward_hip(self, x, layers, encode_only):
        from .... import engine
        cfg = self._cfg
        if cfg["norm"] not in ("instance", "batch") or cfg["padding_type"] != "reflect" or cfg["use_dropout"]:
            raise NotImplementedError("HIP generator supports norm instance|batch, reflect padding, no dropout")
        if self.training and cfg["norm"] == "batch":
            raise NotImplementedError("HIP generator is inference-only: call .eval() (BatchNorm uses running statistics)")
        last = len(self.model) - 1
        taps = tuple(sorted({l for l in layers if l != -1 and l <= last}))
        unavailable = [t for t in taps if t in (0, last - 2)]
        if unavailable:
            raise NotImplementedError("feature taps %s (reflection-padded tensors) are not materialised on the HIP path" % unavailable)
        self._hip_check_inference()
        prec = self._hip_precision()
        if encode_only and taps and layers[-1] == taps[-1] < last - 2 and self.hip_encoder_graph:
            # the reference returns at the last requested layer (:328-329): a graph of its own that ends there, cached beside the full one
            net = self._hip_net(("gen_enc", taps, prec), lambda sd, dev: engine.build_generator(sd, dev, taps=taps, precision=prec, norm=cfg["norm"],
                                                                                               stop_after_taps=True))
            outs = net.forward(x)
            return [outs[net.tap_slots[t]] for t in layers if t in net.tap_slots]
        net = self._hip_net(("gen", taps, prec), lambda sd, dev: engine.build_generator(sd, dev, taps=taps, precision=prec, norm=cfg["norm"]))
        outs = net.forward(x)
        out = outs[net.out_slot]
        if not layers:
            return out
        feats = [outs[net.tap_slots[t]] for t in layers if t in net.tap_slots]
        if encode_only and layers[-1] in net.tap_slots:
            return feats
        return out, feats


class UnetSkipConnectionBlock(nn.Module):
    """One level of the U-Net: ``cat([x, up(submodule(down(x)))], 1)`` (the outermost level returns ``up(..)`` alone).  down = [LeakyReLU(0.2, inplace)]
    Conv2d(k4, s2, p1) [norm]; up = ReLU ConvTranspose2d(k4, s2, p1) [norm] -- outermost: no down activation, no norms, Tanh last, a biased
    up-convolution; innermost: no down norm, an up-convolution of one tensor.  The LeakyReLU is IN PLACE, as in the reference: it alters ``x``
    before the concatenation, so the skip half of what a block returns is ``leaky(x)`` (p2p_networks.py:199, :236)."""

    def __init__(self, outer_nc, inner_nc, input_nc=None, submodule=None, outermost=False, innermost=False, norm_layer="batch", use_dropout=False,
                 track_running_stats=True):
        super().__init__()
        self.outermost = outermost
        norm_layer = get_norm_layer(norm_layer, track_running_stats)
        base = norm_layer.func if isinstance(norm_layer, functools.partial) else norm_layer
        use_bias = base == nn.InstanceNorm2d
        if input_nc is None:
            input_nc = outer_nc
        downconv = nn.Conv2d(input_nc, inner_nc, kernel_size=4, stride=2, padding=1, bias=use_bias)
        downrelu = nn.LeakyReLU(0.2, True)
        downnorm = norm_layer(inner_nc)
        uprelu = nn.ReLU(True)
        upnorm = norm_layer(outer_nc)
        if outermost:
            upconv = nn.ConvTranspose2d(inner_nc * 2, outer_nc, kernel_size=4, stride=2, padding=1)
            model = [downconv] + [submodule] + [uprelu, upconv, nn.Tanh()]
        elif innermost:
            upconv = nn.ConvTranspose2d(inner_nc, outer_nc, kernel_size=4, stride=2, padding=1, bias=use_bias)
            model = [downrelu, downconv] + [uprelu, upconv, upnorm]
        else:
            upconv = nn.ConvTranspose2d(inner_nc * 2, outer_nc, kernel_size=4, stride=2, padding=1, bias=use_bias)
            model = [downrelu, downconv, downnorm] + [submodule] + [uprelu, upconv, upnorm]
            if use_dropout:
                model = model + [nn.Dropout(0.5)]
        self.model = nn.Sequential(*model)

    def forward(self, x):
        if self.outermost:
            return self.model(x)
        return torch.cat([x, self.model(x)], 1)


class UnetGenerator(HipBacked, nn.Module):
    """pix2pix U-Net generator: ``num_downs`` levels of UnetSkipConnectionBlock, widths ngf, 2 ngf, 4 ngf, 8 ngf, 8 ngf, ..; the module tree (and so
    every state-dict key, ``model.model.0.weight`` ..) is the reference's.  H and W must be divisible by 2^num_downs (the reference fails in torch.cat
    otherwise; the ``reflectpad_divisible`` wrapper pads to that).  On a HIP device the forward is inference only
    (gandtr_amd.engine.build_unet_generator); Dropout is the identity there, as in eval mode."""

    #: single-pass fp16; NOT covered by the generators' 1e-3 contract ("The U-Net generator"): "f16x3" is the exact mode that is;
    #: the compensated generator modes "f16c" / "f16ch" do not exist here
    hip_default_precision = "f16"

    def __init__(self, input_nc, output_nc, num_downs, ngf=64, norm_layer="batch", use_dropout=False, track_running_stats=True):
        super().__init__()
        if num_downs < 5:
            raise ValueError("a UnetGenerator has at least 5 levels, got num_downs = %s" % (num_downs,))
        self.meta = {"in_channels": input_nc, "out_channels": output_nc}
        self._cfg = dict(norm=norm_layer if isinstance(norm_layer, str) else None, num_downs=num_downs, ngf=ngf)
        kw = dict(norm_layer=norm_layer, track_running_stats=track_running_stats)
        block = UnetSkipConnectionBlock(ngf * 8, ngf * 8, innermost=True, **kw)
        for _ in range(num_downs - 5):
            block = UnetSkipConnectionBlock(ngf * 8, ngf * 8, submodule=block, use_dropout=use_dropout, **kw)
        block = UnetSkipConnectionBlock(ngf * 4, ngf * 8, submodule=block, **kw)
        block = UnetSkipConnectionBlock(ngf * 2, ngf * 4, submodule=block, **kw)
        block = UnetSkipConnectionBlock(ngf, ngf * 2, submodule=block, **kw)
        self.model = UnetSkipConnectionBlock(output_nc, ngf, input_nc=input_nc, submodule=block, outermost=True, **kw)

    def forward(self, input):
        if self._hip_device().type == "cuda":
            return self._forward_hip(input)
        return self.model(input)

    def _hip_modes(self):
        """the precision of the HIP forward, checked: the U-Net runs in 'f16' or 'f16x3'"""
        prec = self._hip_precision()
        if prec not in ("f16", "f16x3"):
            raise NotImplementedError("HIP U-Net generator runs in 'f16' or 'f16x3'; %r is a ResnetGenerator mode" % (prec,))
        return prec

    def _forward_hip(self, x):
        from .... import engine
        cfg = self._cfg
        if cfg["norm"] not in ("instance", "batch"):
            raise NotImplementedError("HIP U-Net generator supports norm instance|batch")
        if self.training and cfg["norm"] == "batch":
            raise NotImplementedError("HIP U-Net generator is inference-only: call .eval() (BatchNorm uses running statistics)")
        prec = self._hip_modes()
        div = 2 ** cfg["num_downs"]
        if x.dim() != 4 or x.shape[2] % div or x.shape[3] % div:
            raise ValueError("a UnetGenerator with num_downs = %d needs H and W divisible by %d, got %s: pad the input with the "
                             "'reflectpad_divisible:%d' wrapper" % (cfg["num_downs"], div, tuple(x.shape), div))
        self._hip_check_inference()
        net = self._hip_net(("unet", prec), lambda sd, dev: engine.build_unet_generator(sd, dev, precision=prec, norm=cfg["norm"]))
        return net.forward(x)[net.out_slot]


class NLayerDiscriminator(HipBacked, nn.Module):
    """PatchGAN discriminator: Conv(k4, s2, p1) + LeakyReLU(0.2), n_layers - 1 times Conv(k4, s2, p1) + norm + LeakyReLU(0.2) with widths
    ndf * min(2^n, 8), one Conv(k4, s1, p1) + norm + LeakyReLU(0.2), Conv(k4, s1, p1) to ONE channel: a map of per-patch logits.  The nn.Sequential
    tree is the reference's (``model.0.weight`` ..).  On a HIP device the forward is inference only (gandtr_amd.engine.build_discriminator); only the
    ``no_antialias`` configuration with 4x4 kernels exists, on any device."""

    #: single-pass fp16 like HED and the embedders; "f16x3" is the exact mode, the generator modes "f16c" / "f16ch" do not exist here
    hip_default_precision = "f16"

    def __init__(self, input_nc, ndf=64, n_layers=3, kw=4, norm_layer="batch", no_antialias=True, track_running_stats=True):
        super().__init__()
        if not no_antialias:
            raise NotImplementedError("anti-aliased down-sampling (CUT) is outside the gandtr hot path")
        if kw != 4:
            raise NotImplementedError("PatchGAN kernel size [%s] is not implemented (4 only)" % (kw,))
        self.meta = {"in_channels": input_nc, "out_channels": 1}
        self._cfg = dict(norm=norm_layer if isinstance(norm_layer, str) else None, ndf=ndf)
        norm_layer = get_norm_layer(norm_layer, track_running_stats)
        base = norm_layer.func if isinstance(norm_layer, functools.partial) else norm_layer
        use_bias = base == nn.InstanceNorm2d

        padw = 1
        sequence = [nn.Conv2d(input_nc, ndf, kernel_size=kw, stride=2, padding=padw), nn.LeakyReLU(0.2, True)]
        nf_mult = 1
        for n in range(1, n_layers):
            nf_mult_prev, nf_mult = nf_mult, min(2 ** n, 8)
            sequence += [nn.Conv2d(ndf * nf_mult_prev, ndf * nf_mult, kernel_size=kw, stride=2, padding=padw, bias=use_bias),
                         norm_layer(ndf * nf_mult), nn.LeakyReLU(0.2, True)]
        nf_mult_prev, nf_mult = nf_mult, min(2 ** n_layers, 8)
        sequence += [nn.Conv2d(ndf * nf_mult_prev, ndf * nf_mult, kernel_size=kw, stride=1, padding=padw, bias=use_bias),
                     norm_layer(ndf * nf_mult), nn.LeakyReLU(0.2, True)]
        sequence += [nn.Conv2d(ndf * nf_mult, 1, kernel_size=kw, stride=1, padding=padw)]
        self.model = nn.Sequential(*sequence)

    def forward(self, input):
        if self._hip_device().type == "cuda":
            return self._forward_hip(input)
        return self.model(input)

    def forward_multi(self, input):
        return self.forward(input)

    def _forward_hip(self, x):
        from .... import engine
        cfg = self._cfg
        if cfg["norm"] not in ("instance", "batch"):
            raise NotImplementedError("HIP discriminator supports norm instance|batch")
        if self.training and cfg["norm"] == "batch":
            raise NotImplementedError("HIP discriminator is inference-only: call .eval() (BatchNorm uses running statistics)")
        self._hip_check_inference()
        prec = self._hip_precision()
        if prec not in ("f16", "f16x3"):
            raise NotImplementedError("HIP discriminator runs in 'f16' or 'f16x3'; %r is a generator mode" % (prec,))
        net = self._hip_net(("disc", prec), lambda sd, dev: engine.build_discriminator(sd, dev, precision=prec, norm=cfg["norm"]))
        return net.forward(x)[net.out_slot]


class Normalize(nn.Module):
    """x / (sum(x^power, dim 1)^(1 / power) + 1e-7)"""

    def __init__(self, power=2):
        super().__init__()
        self.power = power

    def forward(self, x):
        norm = x.pow(self.power).sum(1, keepdim=True).pow(1. / self.power)
        return x.div(norm + 1e-7)


UNAVAILABLE_TAPS = "feature taps %s (reflection-padded tensors) are not materialised on the HIP path"


def generator_tap_channels(layers, ngf=64, n_blocks=9, input_nc=3, output_nc=3, no_antialias=True, no_antialias_up=True):
    """channel counts of the taps ``layers`` (nn.Sequential indices) of a ResnetGenerator, from its layout alone: no forward.  The two reflection-padded
    tensors (index 0 and the pad before the head) are refused like ResnetGenerator refuses them on the HIP path.  ``no_antialias`` False: a Downsample
    behind each down layer; ``no_antialias_up`` False: an Upsample (of the incoming width) in front of each up conv."""
    down = 3 if no_antialias else 4
    up = lambda cin: [cin // 2] * 3 if no_antialias_up else [cin] + [cin // 2] * 3
    widths = ([input_nc] + [ngf] * 3 + [2 * ngf] * down + [4 * ngf] * down + [4 * ngf] * n_blocks + up(4 * ngf) + up(2 * ngf) + [ngf] +
              [output_nc] * 2)
    last = len(widths) - 1
    bad = [l for l in layers if l in (0, last - 2)]
    if bad:
        raise NotImplementedError(UNAVAILABLE_TAPS % bad)
    out = [l for l in layers if not 0 <= l <= last]
    if out:
        raise ValueError("a ResnetGenerator with %d blocks has the layers 0 .. %d, got %s" % (n_blocks, last, out))
    return [widths[l] for l in layers]


class PatchSampleF(HipBacked, nn.Module):
    """CUT's ``featdown`` network: per feature map, ``num_patches`` positions (the same for every image of the batch) -> rows [B * P][C] -> optional
    Linear(C, nc) -> ReLU -> Linear(nc, nc) -> l2 normalisation.  Attribute names and state-dict keys (``mlp_<i>.0.weight`` ..) are the reference's.

    Unlike the reference's constructor this one runs no generator forward and needs no GPU: with ``input_nc`` and ``nce_layers`` given, the MLPs' input
    widths come from the layout of the 9-block ResnetGenerator the reference assumes (generator_tap_channels) and the MLPs are created on the CPU; without
    them the MLPs are created at the first forward on the features' device (``create_mlp``).  On HIP tensors all layers run in ONE launch of
    gdt_patch_sample (gandtr_amd/csrc/patch_nce.hip), inference only; on CPU tensors the reference's torch ops run."""

    def __init__(self, use_mlp=True, init_type="normal", init_gain=0.02, input_nc=3, nc=256, nce_layers="0,4,8,12,16"):
        super().__init__()
        self.meta = {"in_channels": input_nc, "out_channels": nc}
        self._disable_graphviz = True
        self.l2norm = Normalize(2)
        self.use_mlp = use_mlp
        self.nc = nc
        self.mlp_init = False
        self.init_type = init_type
        self.init_gain = init_gain
        if input_nc and nce_layers:
            layers = [int(i) for i in nce_layers.split(",")] if isinstance(nce_layers, str) else [int(i) for i in nce_layers]
            self._create_mlp_widths(generator_tap_channels(layers, input_nc=input_nc), "cpu")

    def _create_mlp_widths(self, widths, device):
        for mlp_id, width in enumerate(widths):
            mlp = nn.Sequential(nn.Linear(width, self.nc), nn.ReLU(), nn.Linear(self.nc, self.nc))
            setattr(self, "mlp_%d" % mlp_id, mlp.to(device))
        self.mlp_init = True

    def create_mlp(self, feats, device=None):
        """one MLP per feature map, on ``device`` or else where the features are (the reference's ``.cuda()`` default, without requiring a GPU)"""
        self._create_mlp_widths([feat.shape[1] for feat in feats], device if device else feats[0].device)

    def forward(self, feats, num_patches=64, patch_ids=None, device=None):
        if self.use_mlp and not self.mlp_init:
            self.create_mlp(feats, device)
        if feats and feats[0].is_cuda:
            return self._forward_hip(feats, num_patches, patch_ids)
        return_ids, return_feats = [], []
        for feat_id, feat in enumerate(feats):
            B, H, W = feat.shape[0], feat.shape[2], feat.shape[3]
            feat_reshape = feat.permute(0, 2, 3, 1).flatten(1, 2)
            if num_patches > 0:
                if patch_ids is not None:
                    patch_id = patch_ids[feat_id]
                else:
                    patch_id = np.random.permutation(feat_reshape.shape[1])
                    patch_id = patch_id[:int(min(num_patches, patch_id.shape[0]))]
                patch_id = torch.as_tensor(patch_id, dtype=torch.long, device=feat.device)
                x_sample = feat_reshape[:, patch_id, :].flatten(0, 1)
            else:
                x_sample = feat_reshape
                patch_id = []
            if self.use_mlp:
                x_sample = getattr(self, "mlp_%d" % feat_id)(x_sample)
            return_ids.append(patch_id)
            x_sample = self.l2norm(x_sample)
            if num_patches == 0:
                x_sample = x_sample.permute(0, 2, 1).reshape([B, x_sample.shape[-1], H, W])
            return_feats.append(x_sample)
        return return_feats, return_ids

    def _forward_hip(self, feats, num_patches, patch_ids):
        from .... import _hip
        if num_patches == 0:
            raise NotImplementedError("num_patches == 0 (whole-map output) is not provided on the HIP path")
        if len(feats) > _hip.PATCH_MAX_LAYERS:
            raise NotImplementedError("the HIP path samples at most %d feature maps per call" % _hip.PATCH_MAX_LAYERS)
        self._hip_check_inference()
        lib = _hip.load()
        dev = feats[0].device
        feats = [f.detach().contiguous().float() for f in feats]
        # position ids: drawn like the reference draws them (per layer, in layer order), or taken; host ids are checked and uploaded as ONE table
        ids, host = [None] * len(feats), {}
        for i, f in enumerate(feats):
            hw = f.shape[2] * f.shape[3]
            if patch_ids is None:
                pid = np.random.permutation(hw)
                pid = pid[:int(min(num_patches, pid.shape[0]))]
            else:
                pid = patch_ids[i]
            if torch.is_tensor(pid) and pid.is_cuda:
                ids[i] = pid.to(dev).reshape(-1)                # a device table is trusted (gdt_patch_sample)
            else:
                pid = np.asarray(pid.cpu() if torch.is_tensor(pid) else pid).reshape(-1)
                if pid.size < 1 or pid.size > hw or pid.min() < 0 or pid.max() >= hw:
                    raise ValueError("patch ids of feature map %d: 1 .. %d ids in [0, %d)" % (i, hw, hw))
                host[i] = pid.astype(np.int32)
        with torch.cuda.device(dev):
            if host:
                table = torch.from_numpy(np.concatenate([host[i] for i in sorted(host)])).to(dev)
                at = 0
                for i in sorted(host):
                    ids[i] = table[at:at + host[i].size]
                    at += host[i].size
            ids32 = [t if t.dtype == torch.int32 else t.to(torch.int32) for t in ids]
            widths = [self.nc if self.use_mlp else f.shape[1] for f in feats]
            rows = [f.shape[0] * t.numel() for f, t in zip(feats, ids32)]
            flat = torch.empty(sum(r * w for r, w in zip(rows, widths)), dtype=torch.float32, device=dev)
            outs, at = [], 0
            for r, w in zip(rows, widths):
                outs.append(flat[at:at + r * w].view(r, w))
                at += r * w
            table, keep = (_hip.PatchLayer * len(feats))(), []
            for i, (f, t, o) in enumerate(zip(feats, ids32, outs)):
                ptrs = [None] * 4
                if self.use_mlp:
                    mlp = getattr(self, "mlp_%d" % i)
                    if mlp[0].in_features != f.shape[1]:
                        raise ValueError("feature map %d has %d channels, mlp_%d takes %d" % (i, f.shape[1], i, mlp[0].in_features))
                    ws = [p.detach().contiguous().float() for p in (mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias)]
                    if any(w.device != dev for w in ws):
                        raise ValueError("mlp_%d is on %s, the features on %s" % (i, ws[0].device, dev))
                    keep.append(ws)
                    ptrs = [w.data_ptr() for w in ws]
                table[i] = _hip.PatchLayer(f.data_ptr(), t.data_ptr(), ptrs[0], ptrs[1], ptrs[2], ptrs[3], o.data_ptr(), f.shape[0], f.shape[1],
                                           f.shape[2] * f.shape[3], t.numel())
            _hip.check(lib.gdt_patch_sample(table, len(feats), int(self.nc) if self.use_mlp else 0, int(bool(self.use_mlp)),
                                            torch.cuda.current_stream(dev).cuda_stream))
        return outs, [t.long() for t in ids]
