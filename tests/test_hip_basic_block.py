"""GPU parity of the fused identity BasicBlock (conv3x3_basic.hip: conv 3x3 + ReLU -> conv 3x3 + residual + ReLU, 64 -> 64 channels, torchvision's BasicBlock
as restated in components/model/network/backbones.py, one launch, variant 936064) against float64 under the derived bound of tests/conv_bound.py: every
output element, the image borders included (the second conv zero-pads h, not x: a ring computed from zero-padded x shows there), the second block on
the first one's actual output; bit-identical between runs and between batch positions; and the layer-by-layer route of the same build under the bound
of its own chain.

The bound: h = layer(x) is rounded to fp16 once (in LDS), so its bound is the input perturbation of the second conv (in_delta); conv_bound's residual term
allows a rounding before the residual is added, which the fused kernel does not make (it adds x in fp32 and rounds once) and the layer-by-layer epilogue does.

MEASURED (MI355X), max |d| / bound of block 1 / block 2 (the bound is mostly h's fp16 rounding carried through the second conv, which a kernel reaches only
where many roundings line up: ratios near 0.3 are what a correct kernel shows); the border rows and columns print the same or smaller figures:
    bn   (2, 5, 5)    fused 0.275 / 0.277   layer by layer 0.275 / 0.271
    bias (2, 5, 5)    fused 0.266 / 0.249   layer by layer 0.283 / 0.233
    bn   (1, 16, 16)  fused 0.262 / 0.243   layer by layer 0.283 / 0.264
    bias (1, 16, 16)  fused 0.272 / 0.247   layer by layer 0.297 / 0.226
    bn   (3, 33, 17)  fused 0.274 / 0.233   layer by layer 0.283 / 0.261
    bias (3, 33, 17)  fused 0.275 / 0.245   layer by layer 0.275 / 0.248
    bn   (2, 37, 45)  fused 0.313 / 0.298   layer by layer 0.313 / 0.305
    bias (2, 37, 45)  fused 0.277 / 0.236   layer by layer 0.277 / 0.282
    bn   (2, 64, 48)  fused 0.258 / 0.245   layer by layer 0.255 / 0.238
    bias (2, 64, 48)  fused 0.285 / 0.226   layer by layer 0.285 / 0.309
"""
import pytest
import torch

import conv_bound as cb
from gandtr_amd.engine import HipNet
from gandtr_amd.tools import synth

pytestmark = pytest.mark.gpu

FUSED = 936064
SHAPES = [(2, 5, 5),        # map smaller than a patch; every ring pixel is padding
          (1, 16, 16),      # exactly one patch
          (3, 33, 17),      # one pixel over, in both directions
          (2, 37, 45),      # ragged right and bottom patches
          (2, 64, 48)]      # whole patches, interior seams


def _g(name, shape, std):
    return synth._normal(0, name, shape, std)


def _bn_of(name, c):
    sd = {}
    synth._bn(sd, 0, name, c)
    return tuple(sd[name + k] for k in (".weight", ".bias", ".running_mean", ".running_var"))


def _block_net(dev, norm, nblocks=2):
    """3 -> 64 by a 1x1 conv (tapped: the fp16 block input), then ``nblocks`` identity BasicBlocks, each output tapped; ``norm`` "bn": bias-free convs
    with a BatchNorm (folded at pack time), "bias": plain biases"""
    net = HipNet(dev, "f16")
    t = net.input(3)
    x = net.conv(t, _g("w0", (64, 3, 1, 1), 0.5), _g("b0", (64,), 0.3), relu=True)
    taps, ws = [net.output_nchw(x)], []
    for b in range(nblocks):
        w1, w2 = _g("w1%d" % b, (64, 64, 3, 3), 576 ** -0.5), _g("w2%d" % b, (64, 64, 3, 3), 576 ** -0.5)
        if norm == "bn":
            b1 = b2 = None
            bn1, bn2 = _bn_of("bn1%d" % b, 64), _bn_of("bn2%d" % b, 64)
        else:
            b1, b2 = _g("b1%d" % b, (64,), 0.2), _g("b2%d" % b, (64,), 0.2)
            bn1 = bn2 = None
        h = net.conv(x, w1, b1, bn=bn1, pad=1, relu=True)
        x = net.conv(h, w2, b2, bn=bn2, pad=1, relu=True, residual=x)
        taps.append(net.output_nchw(x))
        ws.append((w1, b1, bn1, w2, b2, bn2))
    net.finalize()
    return net, taps, ws


def _block_bound(x, w):
    """float64 reference and per-output bound of one block on the fp16 input ``x`` (the issue's chain)"""
    w1, b1, bn1, w2, b2, bn2 = w
    h = cb.layer(x, *cb.fold(w1, b1, bn1), pad=1, act="relu")
    return cb.layer(h.ref, *cb.fold(w2, b2, bn2), pad=1, act="relu", residual=x, in_delta=h.bound)


def _run(dev, norm, x):
    net, taps, ws = _block_net(dev, norm)
    net.set_profiling(True)
    outs = net.forward(x.to(dev))
    torch.cuda.synchronize()
    variants = [v for k, v, ms, fl in net.profile() if k == 1]
    return net, taps, ws, outs, variants


@pytest.mark.parametrize("norm", ["bn", "bias"])
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_fused_basic_block(cuda_device, norm, n, h, w, monkeypatch):
    monkeypatch.setenv("GDT_CONV_BASIC", "2")                         # read when a net plans a geometry: wherever the shapes fit, whatever the patch count
    x = synth.synth_input(5, (n, 3, h, w))
    net, taps, ws, outs, variants = _run(cuda_device, norm, x)
    assert variants.count(FUSED) == 2, variants                       # both blocks ran as one launch each
    xin = outs[taps[0]].double().cpu()
    got1, got2 = outs[taps[1]].double().cpu(), outs[taps[2]].double().cpu()
    r1 = _block_bound(xin, ws[0])
    r2 = _block_bound(got1, ws[1])                                    # the second block on the first one's actual (fp16) output
    label = "936064 %s %s" % (norm, (n, h, w))
    cb.assert_within(got1, r1, label + " block 1")
    cb.assert_within(got2, r2, label + " block 2")
    # border rows and columns under the same bound (part of the above; printed on their own: a wrongly padded h shows here)
    for name, sl in (("top", (slice(None), slice(None), slice(0, 1))), ("bottom", (slice(None), slice(None), slice(h - 1, h))),
                     ("left", (slice(None), slice(None), slice(None), slice(0, 1))), ("right", (slice(None), slice(None), slice(None), slice(w - 1, w)))):
        q = float(((got1[sl] - r1.ref[sl]).abs() / r1.bound[sl]).max())
        print("%s block 1 %s border: max |d| / bound = %.3f" % (label, name, q))
        assert q <= 1.0, (label, name, q)
    again = net.forward(x.to(cuda_device))
    assert torch.equal(outs[taps[1]], again[taps[1]]) and torch.equal(outs[taps[2]], again[taps[2]])       # deterministic
    # the layer-by-layer route of the same build: the code is absent, its result meets the bound of its own chain (not bitwise the fused one's)
    monkeypatch.setenv("GDT_CONV_BASIC", "0")
    _, taps0, _, outs0, variants0 = _run(cuda_device, norm, x)
    assert FUSED not in variants0, variants0
    assert torch.equal(outs0[taps0[0]], outs[taps[0]])                # (the block input does not depend on the route)
    l1 = outs0[taps0[1]].double().cpu()
    cb.assert_within(l1, r1, label + " block 1 layer by layer")
    cb.assert_within(outs0[taps0[2]].double().cpu(), _block_bound(l1, ws[1]), label + " block 2 layer by layer")


@pytest.mark.parametrize("norm", ["bn", "bias"])
def test_an_image_does_not_depend_on_its_batch_position(cuda_device, norm, monkeypatch):
    """image 0 of a batch of 3 equals the same image run alone, bit for bit (and so does the last one)"""
    monkeypatch.setenv("GDT_CONV_BASIC", "2")
    x = synth.synth_input(7, (3, 3, 33, 17))
    net, taps, _, outs, variants = _run(cuda_device, norm, x)
    assert variants.count(FUSED) == 2, variants
    for i in (0, 2):
        alone = net.forward(x[i:i + 1].to(cuda_device))
        for t in taps:
            assert torch.equal(alone[t][0], outs[t][i]), (i, t)
