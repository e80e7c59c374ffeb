"""``orig_unet`` on the device: the ConvTranspose2d(k2, s2, p0) layer alone against a float64 transposed convolution under the derived per-element bound of
tests/convt2_bound.py (convt2x2.hip and the generic route of four phase launches), its four sub-pixel phases one by one, every net of
tests/golden/orig_unet.npz against the reference's map in both precisions, the module's forward against the builder's graph, the planner's counter and the
two routes, the ``reflectpad_divisible`` wrapper around the net on the device, the rejected configurations.

Measured figures (MI355X) are in the docstrings of the tests."""
import json
import os

import numpy as np
import pytest
import torch

import conv_bound as CB
import convt2_bound as TB
from gandtr_amd import engine
from gandtr_amd.components.model.network import unet
from gandtr_amd.tools import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "orig_unet.npz"))
CASES = [i for i in range(int(GOLD["n_cases"])) if str(GOLD["c%d_label" % i]) == "orig_unet"]       # (the fixture also holds the outconv_dynint_unet cases)
OUT_CHANNELS = int(GOLD["out_channels"])
KNOB = "GDT_CONVT2X2"
VARIANT = 902128

# (cin, cout, n, h, w), (relu, with_bias) -- a tile of convt2x2.hip is 128 pixel rows (of N H W, in that order) x 128 GEMM columns: 2 x 19 x 21 = 798 rows = six
# whole tiles and one of 30 rows, an odd width, tiles that straddle image rows and the two images; one pixel; the widest layer of the net (16 column tiles, 16
# K chunks) on six pixels; ReLU without bias on a map of 30 rows
LAYERS = [((128, 64, 2, 19, 21), (False, True)), ((128, 64, 1, 1, 1), (False, True)), ((1024, 512, 1, 2, 3), (False, True)), ((256, 128, 2, 5, 3), (True, False))]
GENERIC_ONLY = [(16, 8, 2, 7, 9), (128, 24, 1, 4, 4)]             # channel counts that are no multiples of 64


def _layer_net(dev, shape, relu, with_bias, weight=None, precision="f16"):
    """(net, tap of the input, tap of the layer's output, weight, bias): the input is a 1x1 conv of a 3-channel image (negative values present), tapped as the
    fp16 numbers the layer consumes"""
    cin, cout, n, h, w_ = shape
    net = engine.HipNet(dev, precision)
    a = net.conv(net.input(3), synth._normal(1, "wa", (cin, 3, 1, 1), 0.7), synth._normal(1, "ba", (cin,), 0.2))
    tap = net.output_nchw(a)
    w = CB.f16(synth._normal(2, "wt", (cin, cout, 2, 2), (2.0 / cin) ** 0.5)) if weight is None else weight
    bias = synth._normal(2, "bt", (cout,), 0.1) if with_bias else None
    out = net.output_nchw(net.conv_transposed2(a, w, bias=bias, relu=relu))
    net.finalize()
    return net, tap, out, w, bias


def _profiled(net, x):
    net.set_profiling(True)
    outs = net.forward(x)
    torch.cuda.synchronize()
    variants = [v for k, v, ms, fl in net.profile() if k == 1 and v]
    net.set_profiling(False)
    return outs, variants


def _run_both_routes(net, x, out, monkeypatch, want_kernel):
    """(result of the default route, result with the knob at 0, conv variants of the default route); asserts the planner's count, which kernel ran, and that
    each route is bit-identical run to run"""
    n, _, h, w = x.shape
    monkeypatch.delenv(KNOB, raising=False)
    assert net.convt2x2_launches(n, h, w) == (1 if want_kernel else 0)
    outs, variants = _profiled(net, x)
    assert torch.equal(outs[out], net.forward(x)[out])
    monkeypatch.setenv(KNOB, "0")
    assert net.convt2x2_launches(n, h, w) == 0
    generic, gvariants = _profiled(net, x)
    assert torch.equal(generic[out], net.forward(x)[out])
    monkeypatch.delenv(KNOB)
    assert VARIANT not in gvariants, gvariants
    assert (VARIANT in variants) == want_kernel, variants
    return outs, generic


def _check(got, a, w, bias, relu, label):
    wp, shift = CB.fold(w, bias, transposed=True)
    r = TB.layer(a, wp, shift, relu=relu)
    assert r.K == a.shape[1]
    return CB.assert_within(got, r, label)


@pytest.mark.parametrize("shape,flags", LAYERS, ids=lambda v: "_".join(str(int(e)) for e in v))
def test_layer_against_float64(cuda_device, monkeypatch, shape, flags):
    """convt2x2.hip AND the generic route (four 1 x 1 phase launches) under the derived bound; the two need not be bit-equal; each is bit-identical run to run.
    MEASURED on an MI355X, max |d| / bound, in the order of LAYERS: 0.941, 0.787, 0.475, 0.858, the same on both routes to three digits (the largest ratios are
    the half ulp of the fp16 store, which both routes round alike); generic-only shapes 0.968 (16 -> 8) and 0.865 (128 -> 24)."""
    cin, cout, n, h, w_ = shape
    relu, with_bias = flags
    net, tap, out, w, bias = _layer_net(cuda_device, shape, relu, with_bias)
    assert net.output_shapes(n, h, w_)[out] == (n, cout, 2 * h, 2 * w_)
    x = synth.synth_input(4, (n, 3, h, w_)).to(cuda_device)
    outs, generic = _run_both_routes(net, x, out, monkeypatch, True)
    a = outs[tap].cpu()
    assert torch.equal(CB.f16(a), a) and float(a.min()) < 0
    assert torch.equal(generic[tap].cpu(), a)
    _check(outs[out].cpu(), a, w, bias, relu, "convt2x2 %s relu %d bias %d" % (shape, relu, with_bias))
    _check(generic[out].cpu(), a, w, bias, relu, "generic  %s relu %d bias %d" % (shape, relu, with_bias))


@pytest.mark.parametrize("shape", GENERIC_ONLY, ids=lambda v: "_".join(str(int(e)) for e in v))
def test_generic_only_layer(cuda_device, monkeypatch, shape):
    """channel counts that are no multiples of 64: the generic route whatever the knob says, under the same bound"""
    net, tap, out, w, bias = _layer_net(cuda_device, shape, True, True)
    x = synth.synth_input(5, (shape[2], 3, shape[3], shape[4])).to(cuda_device)
    outs, generic = _run_both_routes(net, x, out, monkeypatch, False)
    assert torch.equal(outs[out], generic[out])
    _check(outs[out].cpu(), outs[tap].cpu(), w, bias, True, "generic-only %s" % (shape,))


def test_layer_f16x3(cuda_device, monkeypatch):
    """the exact mode runs the four phase launches on the split-operand GEMM: 1e-5 of the range against float64 of the fp32 operands.  MEASURED on an
    MI355X: 1.4e-7"""
    monkeypatch.delenv(KNOB, raising=False)
    shape = (128, 64, 2, 5, 7)
    net, tap, out, w, bias = _layer_net(cuda_device, shape, True, True, precision="f16x3")
    x = synth.synth_input(4, (2, 3, 5, 7)).to(cuda_device)
    assert net.convt2x2_launches(2, 5, 7) == 0
    outs = net.forward(x)
    ref = torch.relu(torch.nn.functional.conv_transpose2d(outs[tap].cpu().double(), w.double(), bias.double(), stride=2))
    rel = float((outs[out].cpu().double() - ref).abs().max() / ref.abs().max())
    print("transposed-2 layer f16x3: max|d| / max|ref| = %.3e" % rel)
    assert rel <= 1e-5


@pytest.mark.parametrize("dy,dx", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_phases(cuda_device, monkeypatch, dy, dx):
    """the weight is zero except at kernel tap (dy, dx), no bias: the output is non-zero exactly at the pixels (2y + dy, 2x + dx), on both routes, and there it is
    the layer of that one tap.  MEASURED on an MI355X: max |d| / bound 0.930 for every phase, both routes"""
    shape = (128, 64, 2, 5, 6)
    w = torch.zeros(128, 64, 2, 2)
    w[:, :, dy, dx] = CB.f16(synth._normal(6, "wp", (128, 64), (2.0 / 128) ** 0.5))
    net, tap, out, _, _ = _layer_net(cuda_device, shape, False, False, weight=w)
    x = synth.synth_input(7, (2, 3, 5, 6)).to(cuda_device)
    outs, generic = _run_both_routes(net, x, out, monkeypatch, True)
    a = outs[tap].cpu()
    for name, res in (("convt2x2", outs), ("generic", generic)):
        y = res[out].cpu()
        hit = torch.zeros(10, 12, dtype=torch.bool)
        hit[dy::2, dx::2] = True
        assert bool((y[:, :, ~hit] == 0).all()), name
        assert bool((y[:, :, hit] != 0).all()), name
        _check(y, a, w, None, False, "%s phase (%d, %d)" % (name, dy, dx))


# ------------------------------------------------------------------------------------------------ the whole nets
def _case(i, dev, precision):
    """(module on the device, input, the reference's output, f16_emulated_err)"""
    p = "c%d_" % i
    cfg = json.loads(str(GOLD[p + "cfg"]))
    shape = tuple(int(v) for v in GOLD[p + "shape"])
    wseed, xseed = (int(v) for v in GOLD[p + "seeds"])
    model = unet.CLASSES["orig_unet"](shape[1], OUT_CHANNELS, **cfg).eval()
    model.load_state_dict(synth.orig_unet_state(wseed, in_channels=shape[1], out_channels=OUT_CHANNELS, **cfg), strict=True)
    model.hip_precision = precision
    return model.to(dev), synth.synth_input(xseed, shape, 1.0).to(dev), torch.from_numpy(GOLD[p + "out"]), float(GOLD[p + "f16_emulated_err"])


def _net(model, dev, precision):
    return engine.build_orig_unet({k: v.cpu() for k, v in model.state_dict().items()}, dev, model._cfg, precision=precision)


def _rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("i", CASES)
def test_whole_net_f16(cuda_device, monkeypatch, i):
    """max|d| / max|ref| <= 2 x f16_emulated_err, the family's gate, on both routes of the transposed convs; the planner's count is the number of transposed
    convs and as many launches carry the kernel's profile variant (none with the knob at 0); the forward is bit-identical run to run; the module's forward equals
    the builder's graph bit for bit.  MEASURED on an MI355X, max|d| / max|ref| over f16_emulated_err, cases 0-2: 1.12, 0.93, 0.86 (the same on the generic route;
    max|d| / max|ref| 7.0e-4 .. 1.8e-3)."""
    monkeypatch.delenv(KNOB, raising=False)
    model, x, ref, emu = _case(i, cuda_device, "f16")
    levels = model._cfg["nested_levels"]
    net = _net(model, cuda_device, "f16")
    n, _, h, w = x.shape
    assert net.convt2x2_launches(n, h, w) == levels
    outs, variants = _profiled(net, x)
    on = outs[net.out_slot].cpu()
    assert variants.count(VARIANT) == levels, variants
    assert torch.equal(on, net.forward(x)[net.out_slot].cpu())
    with torch.no_grad():
        y = model(x)
    assert y.is_cuda and y.dtype == torch.float32 and torch.equal(y.cpu(), on)
    monkeypatch.setenv(KNOB, "0")
    assert net.convt2x2_launches(n, h, w) == 0
    outs, gvariants = _profiled(net, x)
    off = outs[net.out_slot].cpu()
    assert VARIANT not in gvariants
    assert torch.equal(off, net.forward(x)[net.out_slot].cpu())
    monkeypatch.delenv(KNOB)
    for name, got in (("convt2x2", on), ("generic", off)):
        assert got.shape == ref.shape
        rel = _rel(got, ref)
        print("case %d orig_unet f16 %s: max|d| / max|ref| = %.3e = %.2f x f16_emulated_err (%.3e)" % (i, name, rel, rel / emu, emu))
        assert rel <= 2 * emu, name


@pytest.mark.parametrize("i", CASES)
def test_whole_net_f16x3(cuda_device, i):
    """1e-5 of max|ref|.  MEASURED on an MI355X, cases 0-2: 5.9e-7, 7.4e-7, 2.4e-6"""
    model, x, ref, _ = _case(i, cuda_device, "f16x3")
    net = _net(model, cuda_device, "f16x3")
    assert net.convt2x2_launches(*x.shape[:1], *x.shape[2:]) == 0
    got = net.forward(x)[net.out_slot].cpu()
    rel = _rel(got, ref)
    print("case %d orig_unet f16x3: max|d| / max|ref| = %.3e" % (i, rel))
    assert rel <= 1e-5
    with torch.no_grad():
        assert torch.equal(model(x).cpu(), got)


def test_wrapped_module_on_the_device(cuda_device, monkeypatch):
    """'reflectpad_divisible:4' around the two-level net on the HIP device at (1, 3, 50, 70) against the reference wrapper + net, under the f16 gate of that run.
    MEASURED on an MI355X: max|d| 1.27e-2, gate 3.29e-2 (max|out| 11.5)."""
    from gandtr_amd.components.data import wrapper
    monkeypatch.delenv(KNOB, raising=False)
    case, div, seed = (int(v) for v in GOLD["wrap_cfg"])
    model, _, _, _ = _case(case, cuda_device, "f16")
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
    print("wrapped orig_unet f16: max|d| = %.3e, gate %.3e" % (d, gate))
    assert d <= gate


def test_rejections(cuda_device):
    model, x, _, _ = _case(2, cuda_device, "f16")                     # nested_levels 4
    with torch.no_grad(), pytest.raises(ValueError, match="divisible by 16.*reflectpad_divisible:16"):
        model(synth.synth_input(1, (1, 4, 40, 48), 1.0).to(cuda_device))
    net = _net(model, cuda_device, "f16")
    with pytest.raises(ValueError):                                   # ... and the graph itself refuses what the module lets through
        net.forward(synth.synth_input(1, (1, 4, 40, 48), 1.0).to(cuda_device))
    for prec in ("f16c", "f16ch"):
        model.hip_precision = prec
        with torch.no_grad(), pytest.raises(NotImplementedError):
            model(x)
    model.hip_precision = "f16"
    model.train()                                                     # no BatchNorm, no Dropout: the forward is the same, but gradients are not recorded
    with pytest.raises(NotImplementedError):
        model(x)
    with torch.no_grad():
        assert model(x).shape == (x.shape[0], OUT_CHANNELS) + tuple(x.shape[2:])
    narrow = unet.OrigUNet(3, 3, nested_levels=1, min_channels=32).eval().to(cuda_device)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="min_channels = 64"):
        narrow(torch.zeros(1, 3, 8, 8, device=cuda_device))
