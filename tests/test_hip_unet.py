"""The pix2pix U-Net generator on the device: ConvTranspose2d(k4, s2, p1) of one tensor or of a concatenation alone against a float64 transposed convolution
under the derived per-element bound of tests/conv_bound.py (conv4x4t_halo.hip and the generic route), the whole network against the reference's map in front of
the Tanh (tests/golden/unet.npz) in both precisions, the planner's counter, the two routes against each other, the ``reflectpad_divisible`` wrapper around the
module on the device, the rejected configurations.

Measured on an MI355X, whole net in f16, max|d| / max|ref| over f16_emulated_err (gate: 2), fixture cases 0-5: 1.40, 0.90, 1.07, 1.20, 0.99, 1.16
(max|d| / max|ref| 9.7e-4, 6.1e-4, 6.6e-4, 5.4e-4, 7.0e-4, 5.8e-4; on the generic route 1.40, 0.90, 1.02, 1.21, 0.98, 1.16); Tanh output max|d| 1.9e-3 .. 4.0e-3 against
gates of 4.3e-3 .. 5.9e-3; f16x3: 3.9e-7 .. 8.9e-7 of the range (gate 1e-5).  Layer test: at most 0.80 of the bound on both routes (generic-only 16-channel shape
0.93, fp32 tanh form 0.001).  Wrapped module: max|d| 3.2e-3, gate 5.9e-3."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_bound as CB
from gandtr_amd import engine
from gandtr_amd.tools import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "unet.npz"))
N_CASES = int(GOLD["n_cases"])
KNOB = "GDT_CONV4X4T_HALO"

# (cin_a, cin_b, cout, n, ih, iw) -- patches of conv4x4t_halo.hip are 8 x 16 input pixels: ragged right and bottom patches among several (19 = 2 * 8 + 3 rows,
# 21 = 16 + 5 columns); one row and one column past a patch; unequal halves on a map smaller than a patch; a single input on a 1 x 1 map (the innermost layer);
# 2 x 2.  Flags (relu_a, relu, with_bn) paired, not crossed: every flag is on and off with one and with two inputs, with one and with several column tiles.
LAYERS = [((64, 64, 64, 2, 19, 21), (True, True, True)), ((64, 64, 64, 2, 19, 21), (False, False, False)),
          ((128, 128, 128, 2, 9, 17), (True, False, True)), ((128, 128, 128, 2, 9, 17), (False, True, False)),
          ((64, 128, 256, 2, 5, 3), (True, True, False)), ((64, 128, 256, 2, 5, 3), (False, False, True)),
          ((128, 0, 64, 2, 1, 1), (False, True, True)), ((128, 0, 64, 2, 1, 1), (True, False, False)),
          ((256, 256, 128, 1, 2, 2), (True, True, True))]
GENERIC_ONLY = (16, 16, 8, 2, 7, 9)
OUTERMOST = (64, 64, 3, 2, 9, 11)


def _layer_net(dev, shape, relu_a, relu, with_bn, out_f32=False):
    """(net, tap of in_a, tap of in_b or None, tap / slot of the layer's output, weight, bias, bn): both inputs are 1x1 convs of a 3-channel image (negative values
    present), tapped as the fp16 numbers the layer consumes"""
    cin_a, cin_b, cout, n, ih, iw = shape
    net = engine.HipNet(dev, "f16")
    t = net.input(3)
    a = net.conv(t, synth._normal(1, "wa", (cin_a, 3, 1, 1), 0.7), synth._normal(1, "ba", (cin_a,), 0.2))
    tap_a = net.output_nchw(a)
    b, tap_b = -1, None
    if cin_b:
        b = net.conv(t, synth._normal(1, "wb", (cin_b, 3, 1, 1), 0.7), synth._normal(1, "bb", (cin_b,), 0.2))
        tap_b = net.output_nchw(b)
    cin = cin_a + cin_b
    w = CB.f16(synth._normal(2, "wt", (cin, cout, 4, 4), (2.0 / (cin * 4)) ** 0.5))
    bias = synth._normal(2, "bt", (cout,), 0.1)
    bn = None
    if with_bn:
        sd = {}
        synth._bn(sd, 3, "bn", cout)
        bn = (sd["bn.weight"], sd["bn.bias"], sd["bn.running_mean"], sd["bn.running_var"])
    if out_f32:
        out = net.conv_transposed4(a, w, b, relu_a=relu_a, bias=bias, out_f32=True, act=1)
    else:
        out = net.output_nchw(net.conv_transposed4(a, w, b, relu_a=relu_a, bias=bias, bn=bn, relu=relu))
    net.finalize()
    return net, tap_a, tap_b, out, w, bias, bn


def _reference(xa, xb, w, bias, bn, relu_a, relu, tanh=False):
    """float64 transposed conv of the tapped fp16 inputs (ReLU on in_a) with the weights AS PACKED (conv_bound.fold: BatchNorm folded in fp32, rounded to fp16) and the
    bound of conv_bound.layer for K = 4 (cin_a + cin_b) products per output: e = g_K mag, + 2^-11 (|ref| + e) + 2^-25 for the fp16 store; the fp32 tanh output
    has no store terms and 2 ulp of tanhf instead"""
    a = F.relu(xa.double()) if relu_a else xa.double()
    if xb is not None:
        a = torch.cat([a, xb.double()], 1)
    wp, shift = CB.fold(w, bias, bn, transposed=True)
    K = 4 * a.shape[1]
    sh = shift[None, :, None, None]
    pre = F.conv_transpose2d(a, wp, None, stride=2, padding=1) + sh
    mag = F.conv_transpose2d(a.abs(), wp.abs(), None, stride=2, padding=1) + sh.abs()
    bound = K * CB.U32 / (1 - K * CB.U32) * mag
    if tanh:
        ref = torch.tanh(pre)
        bound = bound + CB.TANHF_ULPS * 2.0 ** -23 * ref.abs()
    else:
        ref = F.relu(pre) if relu else pre
        bound = bound + CB.U16 * (ref.abs() + bound) + CB.SUB16
    return CB.LayerRef(ref, bound, pre, mag, K)


def _run_both_routes(net, x, out, monkeypatch, want_kernel):
    """(result of the default route, result with the knob at 0, conv variants of the default route); asserts the planner's count and which kernel ran"""
    n, _, ih, iw = x.shape
    monkeypatch.delenv(KNOB, raising=False)
    assert net.conv4x4t_launches(n, ih, iw) == (1 if want_kernel else 0)
    net.set_profiling(True)
    outs = net.forward(x)
    torch.cuda.synchronize()
    variants = [v for k, v, ms, fl in net.profile() if k == 1 and v]
    net.set_profiling(False)
    assert torch.equal(outs[out], net.forward(x)[out])             # bit-identical run to run
    monkeypatch.setenv(KNOB, "0")
    assert net.conv4x4t_launches(n, ih, iw) == 0
    net.set_profiling(True)
    generic = net.forward(x)
    torch.cuda.synchronize()
    gvariants = [v for k, v, ms, fl in net.profile() if k == 1 and v]
    net.set_profiling(False)
    monkeypatch.delenv(KNOB)
    assert not any(907000 <= v < 908000 for v in gvariants), gvariants
    return outs, generic, variants


@pytest.mark.parametrize("shape,flags", LAYERS, ids=lambda v: "_".join(str(int(e)) for e in v))
def test_layer_against_float64(cuda_device, monkeypatch, shape, flags):
    """per output element |got - ref| <= bound (see _reference) for conv4x4t_halo.hip AND for the generic route (copy of the concatenation + four phase launches);
    the two need not be bit-equal.  MEASURED on an MI355X, max |d| / bound: 0.35 .. 0.80, the same on both routes to three digits (the largest ratios are the
    half ulp of the fp16 store, which both routes round alike)."""
    cin_a, cin_b, cout, n, ih, iw = shape
    relu_a, relu, with_bn = flags
    net, tap_a, tap_b, out, w, bias, bn = _layer_net(cuda_device, shape, relu_a, relu, with_bn)
    assert net.output_shapes(n, ih, iw)[out] == (n, cout, 2 * ih, 2 * iw)
    x = synth.synth_input(4, (n, 3, ih, iw)).to(cuda_device)
    outs, generic, variants = _run_both_routes(net, x, out, monkeypatch, True)
    assert variants[-1] == 907064, variants
    xa = outs[tap_a].cpu()
    xb = outs[tap_b].cpu() if tap_b is not None else None
    assert torch.equal(CB.f16(xa), xa) and float(xa.min()) < 0
    r = _reference(xa, xb, w, bias, bn, relu_a, relu)
    CB.assert_within(outs[out].cpu(), r, "conv4x4t_halo %s relu_a %d relu %d bn %d" % ((shape,) + tuple(int(f) for f in flags)))
    CB.assert_within(generic[out].cpu(), r, "generic       %s relu_a %d relu %d bn %d" % ((shape,) + tuple(int(f) for f in flags)))


@pytest.mark.parametrize("relu_a,relu,with_bn", [(True, True, True), (False, False, False)])
def test_generic_only_layer(cuda_device, monkeypatch, relu_a, relu, with_bn):
    """cin not a multiple of 64: the generic route whatever the knob says, under the same bound"""
    cin_a, cin_b, cout, n, ih, iw = GENERIC_ONLY
    net, tap_a, tap_b, out, w, bias, bn = _layer_net(cuda_device, GENERIC_ONLY, relu_a, relu, with_bn)
    x = synth.synth_input(5, (n, 3, ih, iw)).to(cuda_device)
    outs, generic, variants = _run_both_routes(net, x, out, monkeypatch, False)
    assert not any(907000 <= v < 908000 for v in variants), variants
    assert torch.equal(outs[out], generic[out])
    r = _reference(outs[tap_a].cpu(), outs[tap_b].cpu(), w, bias, bn, relu_a, relu)
    CB.assert_within(outs[out].cpu(), r, "generic-only %s relu_a %d relu %d bn %d" % (GENERIC_ONLY, relu_a, relu, with_bn))


def test_outermost_form(cuda_device, monkeypatch):
    """cout 3, external fp32 NCHW output, tanh: the generic route; no store terms in the bound, 2 ulp of tanhf instead"""
    cin_a, cin_b, cout, n, ih, iw = OUTERMOST
    net, tap_a, tap_b, out, w, bias, _ = _layer_net(cuda_device, OUTERMOST, True, False, False, out_f32=True)
    assert net.output_shapes(n, ih, iw)[out] == (n, cout, 2 * ih, 2 * iw)
    x = synth.synth_input(6, (n, 3, ih, iw)).to(cuda_device)
    outs, generic, variants = _run_both_routes(net, x, out, monkeypatch, False)
    assert outs[out].dtype == torch.float32 and torch.equal(outs[out], generic[out])
    r = _reference(outs[tap_a].cpu(), outs[tap_b].cpu(), w, bias, None, True, False, tanh=True)
    CB.assert_within(outs[out].cpu(), r, "outermost %s" % (OUTERMOST,))


# ------------------------------------------------------------------------------------------------ the whole net
def _case(i, dev, precision):
    from gandtr_amd.components.model.network import p2p_networks
    p = "c%d_" % i
    num_downs, ngf, dropout, wseed, xseed = (int(v) for v in GOLD[p + "cfg"])
    norm = str(GOLD[p + "norm"])
    model = p2p_networks.UnetGenerator(3, 3, num_downs, ngf=ngf, norm_layer=norm, use_dropout=bool(dropout)).eval()
    model.load_state_dict(synth.unet_state(wseed, norm, ngf=ngf, num_downs=num_downs, gain=float(GOLD["gain"])))
    model.hip_precision = precision
    x = synth.synth_input(xseed, tuple(int(v) for v in GOLD[p + "shape"]), 1.0)
    return model.to(dev), x.to(dev), torch.from_numpy(GOLD[p + "pre"]), float(GOLD[p + "f16_emulated_err"]), p


def _pre_tanh_net(model, dev, precision):
    return engine.build_unet_generator({k: v.cpu() for k, v in model.state_dict().items()}, dev, precision=precision, pre_tanh=True, norm=model._cfg["norm"])


def _expected_kernel_launches(ngf, num_downs):
    """up convs with cin_a, cin_b and cout multiples of 64 (the outermost, cout 3, never): level i reads 2 x width_i (the innermost 1 x) and writes width_(i-1)"""
    widths = [ngf * min(2 ** i, 8) for i in range(num_downs)]
    return sum(1 for i in range(1, num_downs) if widths[i] % 64 == 0 and widths[i - 1] % 64 == 0)


@pytest.mark.parametrize("i", range(N_CASES))
def test_whole_net_f16(cuda_device, monkeypatch, i):
    """map in front of the Tanh: max|d| / max|ref| <= 2 x f16_emulated_err (the emulation rounds conv inputs and BatchNorm-folded weights to fp16; the factor 2, the
    project's gate for the discriminator, covers the summation order and the rounding points the emulation lacks: the fp16 store of a conv output that feeds an
    InstanceNorm); the Tanh output of the module within the same ABSOLUTE figure (|tanh'| <= 1).
    MEASURED on an MI355X, max|d| / max|ref| over f16_emulated_err, cases 0-5: 1.40, 0.90, 1.07, 1.20, 0.99, 1.16."""
    monkeypatch.delenv(KNOB, raising=False)
    model, x, ref, emu, p = _case(i, cuda_device, "f16")
    net = _pre_tanh_net(model, cuda_device, "f16")
    got = net.forward(x)[net.out_slot].cpu()
    assert got.shape == ref.shape
    rel = float((got - ref).abs().max() / ref.abs().max())
    print("case %d f16: max|d| / max|ref| = %.3e = %.2f x f16_emulated_err (%.3e)" % (i, rel, rel / emu, emu))
    with torch.no_grad():
        y = model(x).cpu()
    d_tanh = float((y[:, :, ::4, ::4] - torch.from_numpy(GOLD[p + "tanh_sub"])).abs().max())
    d_tanh_all = float((y - torch.tanh(ref)).abs().max())
    print("case %d f16: tanh output max|d| = %.3e (every fourth pixel, stored) / %.3e (all, tanh of the stored map); gate %.3e" % (i, d_tanh, d_tanh_all, 2 * emu * float(ref.abs().max())))
    assert rel <= 2 * emu
    assert max(d_tanh, d_tanh_all) <= 2 * emu * float(ref.abs().max())


@pytest.mark.parametrize("i", range(N_CASES))
def test_whole_net_f16x3(cuda_device, i):
    model, x, ref, _, _ = _case(i, cuda_device, "f16x3")
    net = _pre_tanh_net(model, cuda_device, "f16x3")
    got = net.forward(x)[net.out_slot].cpu()
    rel = float((got - ref).abs().max() / ref.abs().max())
    print("case %d f16x3: max|d| / max|ref| = %.3e" % (i, rel))
    assert rel <= 1e-5


@pytest.mark.parametrize("i", range(N_CASES))
def test_routing_and_the_two_routes(cuda_device, monkeypatch, i):
    """the planner's count is the number of up convs whose channel counts are multiples of 64 (0 with the knob at 0; 0 in f16x3); both routes meet the f16 gate,
    and the forward is bit-identical run to run"""
    monkeypatch.delenv(KNOB, raising=False)
    model, x, ref, emu, p = _case(i, cuda_device, "f16")
    num_downs, ngf = int(GOLD[p + "cfg"][0]), int(GOLD[p + "cfg"][1])
    net = _pre_tanh_net(model, cuda_device, "f16")
    n, _, h, w = x.shape
    want = _expected_kernel_launches(ngf, num_downs)
    assert want == {(16, 5): 2, (16, 6): 3, (64, 5): 4, (64, 6): 5}[(ngf, num_downs)]
    assert net.conv4x4t_launches(n, h, w) == want
    net.set_profiling(True)
    on = net.forward(x)[net.out_slot].cpu()
    torch.cuda.synchronize()
    assert sum(1 for k, v, ms, fl in net.profile() if k == 1 and 907000 <= v < 908000) == want
    net.set_profiling(False)
    assert torch.equal(on, net.forward(x)[net.out_slot].cpu())
    monkeypatch.setenv(KNOB, "0")
    assert net.conv4x4t_launches(n, h, w) == 0
    off = net.forward(x)[net.out_slot].cpu()
    assert torch.equal(off, net.forward(x)[net.out_slot].cpu())
    monkeypatch.delenv(KNOB)
    assert _pre_tanh_net(model, cuda_device, "f16x3").conv4x4t_launches(n, h, w) == 0
    for name, y in (("conv4x4t_halo", on), ("generic", off)):
        rel = float((y - ref).abs().max() / ref.abs().max())
        print("case %d %s: %.2f x f16_emulated_err" % (i, name, rel / emu))
        assert rel <= 2 * emu, name


def test_wrapped_module_on_the_device(cuda_device, monkeypatch):
    """'reflectpad_divisible:32' around the module on the HIP device at (1, 3, 50, 70) against the reference wrapper + net, under the f16 gate of that run"""
    from gandtr_amd.components.data import wrapper
    monkeypatch.delenv(KNOB, raising=False)
    model, _, _, _, _ = _case(0, cuda_device, "f16")
    comp = wrapper.initialize_wrappers("reflectpad_divisible:32", cuda_device)
    x = synth.synth_input(80, (1, 3, 50, 70), 1.0)
    with torch.no_grad():
        y = comp(x, model, outputmodel=model)
    assert y.is_cuda and tuple(y.shape) == (1, 3, 50, 70)
    ref = torch.from_numpy(GOLD["wrap_net_out"])
    gate = 2 * float(GOLD["wrap_net_f16_emulated_err"]) * float(GOLD["wrap_net_pre_max"])
    d = float((y.cpu() - ref).abs().max())
    print("wrapped net f16: max|d| = %.3e, gate %.3e" % (d, gate))
    assert d <= gate


def test_rejections(cuda_device):
    model, x, _, _, _ = _case(1, cuda_device, "f16")              # BatchNorm, num_downs 5
    net = model._hip_net(("unet", "f16"), lambda sd, dev: engine.build_unet_generator(sd, dev, precision="f16", norm="batch"))
    bad = synth.synth_input(1, (1, 3, 48, 40), 1.0).to(cuda_device)
    with torch.no_grad(), pytest.raises(ValueError, match="divisible by 32.*reflectpad_divisible"):
        model(bad)
    with pytest.raises(ValueError):                               # ... and the graph itself refuses what the module lets through: the two halves differ in size
        net.forward(synth.synth_input(1, (1, 3, 48, 48), 1.0).to(cuda_device))
    for prec in ("f16c", "f16ch"):
        model.hip_precision = prec
        with torch.no_grad(), pytest.raises(NotImplementedError):
            model(x)
    model.hip_precision = "f16"
    model.train()
    with torch.no_grad(), pytest.raises(NotImplementedError):
        model(x)
