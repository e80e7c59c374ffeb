"""The normalisation U-Nets on the device: the Conv2d of a concatenation alone against a float64 convolution under the derived per-element bound of
tests/conv_bound.py (conv3x3_cat_halo.hip and the generic route), every net of tests/golden/p2p_unet.npz against the reference's map in both precisions, the
module's forward against the builder's graph, the planner's counter, the two routes, the ``reflectpad_divisible`` wrapper around an aligned net on the device,
the rejected configurations.

Measured figures (MI355X) are in the docstrings of the tests."""
import os

import numpy as np
import pytest
import torch

import conv_bound as CB
from gandtr_amd import engine
from gandtr_amd.components.model.network import unet
from gandtr_amd.tools import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "p2p_unet.npz"))
N_CASES = int(GOLD["n_cases"])
OUT_CHANNELS = int(GOLD["out_channels"])
KNOB = "GDT_CONV3X3_CAT_HALO"
INT_ARGS = ("nested_levels", "outconv_kernel", "outconv_channels")

# (cin_a, cin_b, cout, n, h, w) -- patches of conv3x3_cat_halo.hip are 8 x 16 pixels: ragged right and bottom patches among several (19 = 2 * 8 + 3 rows,
# 21 = 16 + 5 columns); one row and one column past a patch; unequal halves on a map smaller than a patch; 1 x 1; 2 x 2.  Flags (relu, with_bn).
LAYERS = [((64, 64, 64, 2, 19, 21), (True, True)), ((64, 64, 64, 2, 19, 21), (False, False)), ((128, 128, 128, 2, 9, 17), (True, False)),
          ((64, 128, 256, 2, 5, 3), (False, True)), ((128, 64, 64, 1, 1, 1), (True, True)), ((256, 256, 128, 1, 2, 2), (True, False))]
GENERIC_ONLY = [((16, 16, 8, 2, 7, 9), 3), ((64, 64, 64, 2, 9, 17), 1)]          # channel counts that are no multiples of 64; a 1x1 kernel


def _layer_net(dev, shape, relu, with_bn, k=3):
    """(net, tap of in_a, tap of in_b, tap of the layer's output, weight, bias, bn): both inputs are 1x1 convs of a 3-channel image (negative values present),
    tapped as the fp16 numbers the layer consumes"""
    cin_a, cin_b, cout, n, h, w_ = shape
    net = engine.HipNet(dev, "f16")
    t = net.input(3)
    a = net.conv(t, synth._normal(1, "wa", (cin_a, 3, 1, 1), 0.7), synth._normal(1, "ba", (cin_a,), 0.2))
    tap_a = net.output_nchw(a)
    b = net.conv(t, synth._normal(1, "wb", (cin_b, 3, 1, 1), 0.7), synth._normal(1, "bb", (cin_b,), 0.2))
    tap_b = net.output_nchw(b)
    cin = cin_a + cin_b
    w = CB.f16(synth._normal(2, "wc", (cout, cin, k, k), (2.0 / (cin * k * k)) ** 0.5))
    bias = synth._normal(2, "bc", (cout,), 0.1)
    bn = None
    if with_bn:
        sd = {}
        synth._bn(sd, 3, "bn", cout)
        bn = (sd["bn.weight"], sd["bn.bias"], sd["bn.running_mean"], sd["bn.running_var"])
    out = net.output_nchw(net.conv_cat(a, b, w, bias=bias, bn=bn, pad=k // 2, relu=relu))
    net.finalize()
    return net, tap_a, tap_b, out, w, bias, bn


def _profiled(net, x):
    net.set_profiling(True)
    outs = net.forward(x)
    torch.cuda.synchronize()
    variants = [v for k, v, ms, fl in net.profile() if k == 1 and v]
    net.set_profiling(False)
    return outs, variants


def _run_both_routes(net, x, out, monkeypatch, want_kernel):
    """(result of the default route, result with the knob at 0, conv variants of the default route); asserts the planner's count and which kernel ran"""
    n, _, h, w = x.shape
    monkeypatch.delenv(KNOB, raising=False)
    assert net.conv3x3_cat_launches(n, h, w) == (1 if want_kernel else 0)
    outs, variants = _profiled(net, x)
    assert torch.equal(outs[out], net.forward(x)[out])             # bit-identical run to run
    monkeypatch.setenv(KNOB, "0")
    assert net.conv3x3_cat_launches(n, h, w) == 0
    generic, gvariants = _profiled(net, x)
    assert torch.equal(generic[out], net.forward(x)[out])
    monkeypatch.delenv(KNOB)
    assert not any(908000 <= v < 909000 for v in gvariants), gvariants
    return outs, generic, variants


def _check(got, xa, xb, w, bias, bn, relu, k, label):
    """per output element |got - ref| <= bound of conv_bound.layer: K = k * k * (cin_a + cin_b) products, the weights as packed (BatchNorm folded in fp32,
    rounded to fp16), one fp16 store"""
    wp, shift = CB.fold(w, bias, bn)
    a = torch.cat([xa, xb], 1)
    assert CB.products(wp) == k * k * a.shape[1]
    return CB.assert_layer(got, a, wp, shift, label, pad=k // 2, act="relu" if relu else None)


@pytest.mark.parametrize("shape,flags", LAYERS, ids=lambda v: "_".join(str(int(e)) for e in v))
def test_layer_against_float64(cuda_device, monkeypatch, shape, flags):
    """conv3x3_cat_halo.hip AND the generic route (copy of the concatenation + the 3x3 conv of one tensor) under the derived bound; the two need not be bit-equal.
    MEASURED on an MI355X, max |d| / bound: 0.09 .. 0.51, the same on both routes to three digits; generic-only shapes 0.73 (16 channels) and 0.92 (1x1 kernel) (the largest ratios are the half ulp of the fp16
    store, which both routes round alike)."""
    cin_a, cin_b, cout, n, h, w_ = shape
    relu, with_bn = flags
    net, tap_a, tap_b, out, w, bias, bn = _layer_net(cuda_device, shape, relu, with_bn)
    assert net.output_shapes(n, h, w_)[out] == (n, cout, h, w_)
    x = synth.synth_input(4, (n, 3, h, w_)).to(cuda_device)
    outs, generic, variants = _run_both_routes(net, x, out, monkeypatch, True)
    assert variants[-1] == 908064, variants
    xa, xb = outs[tap_a].cpu(), outs[tap_b].cpu()
    assert torch.equal(CB.f16(xa), xa) and float(xa.min()) < 0 and float(xb.min()) < 0
    assert torch.equal(generic[tap_a].cpu(), xa) and torch.equal(generic[tap_b].cpu(), xb)
    _check(outs[out].cpu(), xa, xb, w, bias, bn, relu, 3, "conv3x3_cat_halo %s relu %d bn %d" % (shape, relu, with_bn))
    _check(generic[out].cpu(), xa, xb, w, bias, bn, relu, 3, "generic          %s relu %d bn %d" % (shape, relu, with_bn))


@pytest.mark.parametrize("shape,k", GENERIC_ONLY, ids=lambda v: "_".join(str(int(e)) for e in v) if isinstance(v, tuple) else "k%d" % v)
def test_generic_only_layer(cuda_device, monkeypatch, shape, k):
    """channel counts that are no multiples of 64, and a 1x1 kernel: the generic route whatever the knob says, under the same bound"""
    cin_a, cin_b, cout, n, h, w_ = shape
    net, tap_a, tap_b, out, w, bias, bn = _layer_net(cuda_device, shape, True, True, k=k)
    x = synth.synth_input(5, (n, 3, h, w_)).to(cuda_device)
    outs, generic, variants = _run_both_routes(net, x, out, monkeypatch, False)
    assert not any(908000 <= v < 909000 for v in variants), variants
    assert torch.equal(outs[out], generic[out])
    _check(outs[out].cpu(), outs[tap_a].cpu(), outs[tap_b].cpu(), w, bias, bn, True, k, "generic-only %s k %d" % (shape, k))


# ------------------------------------------------------------------------------------------------ the whole nets
def _case(i, dev, precision):
    """(module on the device, its configuration, input, the reference's map, its output, f16_emulated_err, label)"""
    p = "c%d_" % i
    label = str(GOLD[p + "label"])
    cfg = {str(k): (int(v) if str(k) in INT_ARGS else (bool(v) if str(k) == "batchnorm" else float(v))) for k, v in zip(GOLD[p + "cfg_names"], GOLD[p + "cfg_values"])}
    shape = tuple(int(v) for v in GOLD[p + "shape"])
    wseed, xseed = (int(v) for v in GOLD[p + "seeds"])
    model = unet.CLASSES[label](shape[1], OUT_CHANNELS, **cfg).eval()
    model.load_state_dict(synth.p2p_unet_state(label, wseed, in_channels=shape[1], out_channels=OUT_CHANNELS, **cfg), strict=True)
    model.hip_precision = precision
    out = torch.from_numpy(GOLD[p + "out"])
    ref_map = torch.from_numpy(GOLD[p + "pre"]) if int(GOLD[p + "has_tanh"]) else out
    return model.to(dev), synth.synth_input(xseed, shape, 1.0).to(dev), ref_map, out, float(GOLD[p + "f16_emulated_err"]), label


def _map_net(model, dev, precision, pre_act=True):
    return engine.build_p2p_unet(model.label, {k: v.cpu() for k, v in model.state_dict().items()}, dev, model._cfg, precision=precision, pre_act=pre_act)


def _rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("i", range(N_CASES))
def test_whole_net_f16(cuda_device, monkeypatch, i):
    """the map (in front of the Tanh where there is one): max|d| / max|ref| <= 2 x f16_emulated_err, the project's gate for the discriminator and the pix2pix
    U-Net; the module's output -- the Tanh map, where there is one -- within the same ABSOLUTE figure (|tanh'| <= 1), and equal to the builder's graph bit for bit.
    MEASURED on an MI355X, max|d| / max|ref| over f16_emulated_err, cases 0-9: 1.05, 1.12, 1.03, 1.13, 1.13, 0.95, 1.13, 1.06, 0.97, 1.14 (the same on the generic route); module output max|d| 1.6e-3 .. 3.5e-3 against gates of 2.9e-3 .. 6.3e-3."""
    monkeypatch.delenv(KNOB, raising=False)
    model, x, ref, out, emu, label = _case(i, cuda_device, "f16")
    net = _map_net(model, cuda_device, "f16")
    got = net.forward(x)[net.out_slot].cpu()
    assert got.shape == ref.shape
    rel = _rel(got, ref)
    print("case %d %s f16: max|d| / max|ref| = %.3e = %.2f x f16_emulated_err (%.3e)" % (i, label, rel, rel / emu, emu))
    with torch.no_grad():
        y = model(x)
    assert y.is_cuda and y.dtype == torch.float32
    full = _map_net(model, cuda_device, "f16", pre_act=False)
    assert torch.equal(y, full.forward(x)[full.out_slot])
    d_out = float((y.cpu() - out).abs().max())
    print("case %d %s f16: module output max|d| = %.3e; gate %.3e" % (i, label, d_out, 2 * emu * float(ref.abs().max())))
    assert rel <= 2 * emu
    assert d_out <= 2 * emu * float(ref.abs().max())


@pytest.mark.parametrize("i", range(N_CASES))
def test_whole_net_f16x3(cuda_device, i):
    """MEASURED on an MI355X: 4.1e-7 .. 8.7e-7 of the range"""
    model, x, ref, _, _, label = _case(i, cuda_device, "f16x3")
    net = _map_net(model, cuda_device, "f16x3")
    got = net.forward(x)[net.out_slot].cpu()
    rel = _rel(got, ref)
    print("case %d %s f16x3: max|d| / max|ref| = %.3e" % (i, label, rel))
    assert rel <= 1e-5


@pytest.mark.parametrize("i", range(N_CASES))
def test_routing_and_the_two_routes(cuda_device, monkeypatch, i):
    """the planner's count is the number of eligible concatenation convs: 1 for the aligned nets, 0 for every other (0 with the knob at 0; 0 in f16x3), and as
    many launches carry the kernel's profile variant; both routes meet the f16 gate, and the forward is bit-identical run to run"""
    monkeypatch.delenv(KNOB, raising=False)
    model, x, ref, _, emu, label = _case(i, cuda_device, "f16")
    net = _map_net(model, cuda_device, "f16")
    n, _, h, w = x.shape
    want = 1 if label == "aligned_p2p_unet" else 0
    assert net.conv3x3_cat_launches(n, h, w) == want
    outs, variants = _profiled(net, x)
    on = outs[net.out_slot].cpu()
    assert sum(1 for v in variants if 908000 <= v < 909000) == want
    assert torch.equal(on, net.forward(x)[net.out_slot].cpu())
    monkeypatch.setenv(KNOB, "0")
    assert net.conv3x3_cat_launches(n, h, w) == 0
    outs, gvariants = _profiled(net, x)
    off = outs[net.out_slot].cpu()
    assert not any(908000 <= v < 909000 for v in gvariants)
    assert torch.equal(off, net.forward(x)[net.out_slot].cpu())
    monkeypatch.delenv(KNOB)
    assert _map_net(model, cuda_device, "f16x3").conv3x3_cat_launches(n, h, w) == 0
    for name, y in (("conv3x3_cat_halo", on), ("generic", off)):
        rel = _rel(y, ref)
        print("case %d %s %s: %.2f x f16_emulated_err" % (i, label, name, rel / emu))
        assert rel <= 2 * emu, name


def test_wrapped_module_on_the_device(cuda_device, monkeypatch):
    """'reflectpad_divisible:4' around the aligned net (nested_levels 2) on the HIP device at (1, 3, 50, 70) against the reference wrapper + net, under the f16 gate
    of that run.  MEASURED on an MI355X: max|d| 4.0e-3, gate 6.3e-3."""
    from gandtr_amd.components.data import wrapper
    monkeypatch.delenv(KNOB, raising=False)
    case, div, seed = (int(v) for v in GOLD["wrap_cfg"])
    model, _, _, _, _, label = _case(case, cuda_device, "f16")
    assert label == "aligned_p2p_unet"
    x = synth.synth_input(seed, tuple(int(v) for v in GOLD["wrap_shape"]), 1.0)
    with torch.no_grad(), pytest.raises(ValueError, match="reflectpad_divisible:%d" % div):
        model(x.to(cuda_device))
    comp = wrapper.initialize_wrappers("reflectpad_divisible:%d" % div, cuda_device)
    with torch.no_grad():
        y = comp(x, model, outputmodel=model)
    assert y.is_cuda and tuple(y.shape) == tuple(x.shape)
    ref = torch.from_numpy(GOLD["wrap_net_out"])
    gate = 2 * float(GOLD["wrap_net_f16_emulated_err"]) * float(GOLD["wrap_net_map_max"])
    d = float((y.cpu() - ref).abs().max())
    print("wrapped aligned net f16: max|d| = %.3e, gate %.3e" % (d, gate))
    assert d <= gate


def test_rejections(cuda_device):
    model, x, _, _, _, label = _case(1, cuda_device, "f16")              # p2p_unet, nested_levels 5, BatchNorm, dropout 0.5
    bad = synth.synth_input(1, (1, 3, 96, 80), 1.0).to(cuda_device)
    with torch.no_grad(), pytest.raises(ValueError, match="divisible by 64.*reflectpad_divisible:64"):
        model(bad)
    net = _map_net(model, cuda_device, "f16")
    with pytest.raises(ValueError):                               # ... and the graph itself refuses what the module lets through: the two halves differ in size
        net.forward(bad)
    for prec in ("f16c", "f16ch"):
        model.hip_precision = prec
        with torch.no_grad(), pytest.raises(NotImplementedError):
            model(x)
    model.hip_precision = "f16"
    model.train()
    with torch.no_grad(), pytest.raises(NotImplementedError):
        model(x)
    plain, xp, _, _, _, _ = _case(2, cuda_device, "f16")               # outconv_unet without BatchNorm or Dropout: train mode has the same forward
    plain.train()
    with torch.no_grad():
        assert plain(xp).shape == xp.shape
    aligned, xa, _, _, _, _ = _case(7, cuda_device, "f16")             # nested_levels 1: sizes divisible by 2
    with torch.no_grad(), pytest.raises(ValueError, match="divisible by 2.*reflectpad_divisible:2"):
        aligned(synth.synth_input(1, (1, 3, 9, 14), 1.0).to(cuda_device))
