"""The normalisation U-Nets (p2p_unet, outconv_unet, inconv_p2p_unet, aligned_p2p_unet, shallow_p2p_unet) on the host: the registry and the ``mdir`` alias, the
module trees against the reference's key lists and shapes, the CPU forward against the reference's output (tests/golden/p2p_unet.npz), the ``meta`` dicts, what
the device path refuses before it needs a device, and the argument validation of gdt_net_conv with two inputs.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from gandtr_amd import _hip, engine
from gandtr_amd.components.model import network as registry
from gandtr_amd.components.model.network import unet
from gandtr_amd.tools import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "p2p_unet.npz"))
N_CASES = int(GOLD["n_cases"])
DEV = "cuda:0"        # only recorded; no device call happens before finalize()
INT_ARGS = ("nested_levels", "outconv_kernel", "outconv_channels")


def case(i):
    """(label, constructor arguments, input shape, weight seed, input seed) of fixture case i"""
    p = "c%d_" % i
    cfg = {str(k): (int(v) if str(k) in INT_ARGS else (bool(v) if str(k) == "batchnorm" else float(v))) for k, v in zip(GOLD[p + "cfg_names"], GOLD[p + "cfg_values"])}
    wseed, xseed = (int(v) for v in GOLD[p + "seeds"])
    return str(GOLD[p + "label"]), cfg, tuple(int(v) for v in GOLD[p + "shape"]), wseed, xseed


def model_of(i):
    label, cfg, shape, wseed, xseed = case(i)
    model = registry.initialize_model(dict(architecture=label, in_channels=shape[1], out_channels=int(GOLD["out_channels"]), **cfg)).eval()
    sd = synth.p2p_unet_state(label, wseed, in_channels=shape[1], out_channels=int(GOLD["out_channels"]), **cfg)
    return model, sd, synth.synth_input(xseed, shape, 1.0)


def test_registry_and_alias():
    want = {"p2p_unet": unet.P2pUNet, "outconv_unet": unet.OutconvP2pUNet, "inconv_p2p_unet": unet.InconvP2pUNet, "aligned_p2p_unet": unet.AlignedP2pUNet,
            "shallow_p2p_unet": unet.ShallowP2pUNet}
    for label, cls in want.items():
        assert registry.MODEL_LABELS[label] is cls
    import mdir.components.model.network.unet as alias
    assert alias is unet
    for label in ("orig_unet", "outconv_dynint_unet"):                 # not mirrored: the reference's KeyError
        with pytest.raises(KeyError):
            registry.initialize_model({"architecture": label, "in_channels": 3, "out_channels": 3})


def test_constructor_defaults_are_the_references():
    """argument names and defaults of the five constructors (unet.py of the reference)"""
    import inspect
    want = {unet.P2pUNet: dict(dropout=0, conv_opts=None, batchnorm_opts=None, batchnorm=True, nested_levels=7),
            unet.ShallowP2pUNet: dict(conv_opts=None, nested_levels=4),
            unet.OutconvP2pUNet: dict(conv_opts=None, batchnorm_opts=None, nested_levels=7, outconv_channels=32, outconv_kernel=3, dropout=False, batchnorm=False),
            unet.InconvP2pUNet: dict(conv_opts=None, nested_levels=7), unet.AlignedP2pUNet: dict(conv_opts=None, nested_levels=7)}
    for cls, defaults in want.items():
        params = list(inspect.signature(cls.__init__).parameters.values())[1:]
        assert [p.name for p in params[:2]] == ["in_channels", "out_channels"]
        assert {p.name: p.default for p in params[2:]} == defaults, cls


@pytest.mark.parametrize("i", range(N_CASES))
def test_keys_shapes_meta_and_cpu_forward(i):
    """the module tree gives the reference's state-dict keys in its order, with its shapes (a reference checkpoint loads with strict=True); the ``meta`` dict is
    the reference's; the CPU forward with the synthesised weights is the reference's output within 1e-6 of its range (the same torch ops)"""
    p = "c%d_" % i
    model, sd, x = model_of(i)
    keys = [str(k) for k in GOLD[p + "keys"]]
    assert list(model.state_dict().keys()) == keys
    assert [list(v.shape) + [0] * (4 - v.dim()) for v in model.state_dict().values()] == GOLD[p + "shapes"].tolist()
    assert list(sd.keys()) == keys
    model.load_state_dict(sd, strict=True)
    assert model.meta == {str(k): int(v) for k, v in zip(GOLD[p + "meta_names"], GOLD[p + "meta_values"])}
    ref = torch.from_numpy(GOLD[p + "out"])
    with torch.no_grad():
        y = model(x)
    assert y.shape == ref.shape
    d = float((y - ref).abs().max())
    rng = float(ref.max() - ref.min())
    print("case %d: max|d| = %.3e, range %.3f" % (i, d, rng))
    assert d <= 1e-6 * rng


def test_cpu_forward_takes_the_references_other_configurations():
    """conv_opts other than k4 / s2 / p1, BatchNorm options, train mode: plain torch on the CPU"""
    m = unet.OutconvP2pUNet(3, 2, conv_opts={"kernel_size": 2, "padding": 0}, nested_levels=1, batchnorm=True, batchnorm_opts={"track_running_stats": False}, dropout=0.25)
    assert tuple(m(torch.zeros(1, 3, 8, 12)).shape) == (1, 2, 8, 12)
    assert "outerblock.2.nested.3.running_mean" not in m.state_dict() and "outerblock.2.nested.3.weight" in m.state_dict()     # (the innermost block: conv, ReLU, up conv, BatchNorm)
    assert any(isinstance(mod, torch.nn.Dropout) and mod.p == 0.25 for mod in m.modules())
    with pytest.raises(AssertionError):
        unet.OutconvP2pUNet(3, 3, outconv_kernel=4)
    # P2pUNet: Dropout from the fifth block on only, no conv bias but on the last layer
    p = unet.P2pUNet(3, 3, dropout=0.5, nested_levels=6)
    assert sum(isinstance(mod, torch.nn.Dropout) for mod in p.modules()) == 2
    assert [k for k in p.state_dict() if k.endswith(".bias") and p.state_dict()[k].shape == (3,)] == ["outerblock.3.bias"]
    assert p.outerblock[0].bias is None


def _graph(label, finalize=False, precision="f16", sd_edit=None, **cfg):
    in_channels = cfg.pop("in_channels", 3)
    full = unet.family_config(label, in_channels, 3, **cfg)
    sd = synth.p2p_unet_state(label, 0, in_channels=in_channels, out_channels=3, **cfg)
    if sd_edit:
        sd_edit(sd)
    return engine.build_p2p_unet(label, sd, DEV, full, precision=precision, finalize=finalize)


def test_graphs_plan_without_a_device():
    """every fixture case builds and plans: output of the input's size; the planner's count of concatenation convs on conv3x3_cat_halo.hip (1 for the aligned
    nets in f16, 0 elsewhere and in f16x3)"""
    for i in range(N_CASES):
        label, cfg, shape, _, _ = case(i)
        n, c, h, w = shape
        for precision in ("f16", "f16x3"):
            net = _graph(label, precision=precision, in_channels=c, **cfg)
            assert net.output_shapes(n, h, w) == [(n, 3, h, w)]
            assert net.conv3x3_cat_launches(n, h, w) == (1 if label == "aligned_p2p_unet" and precision == "f16" else 0)
    net = _graph("aligned_p2p_unet", nested_levels=2)
    with pytest.raises(ValueError):                               # 18 is not divisible by 4: the two halves of a concatenation differ in size
        net.workspace_bytes(1, 18, 20)


def test_device_path_rejections_that_need_no_device():
    with pytest.raises(NotImplementedError, match="kernel_size 4, stride 2, padding 1"):
        _graph("p2p_unet", nested_levels=2, conv_opts={"kernel_size": 2, "padding": 0})
    with pytest.raises(NotImplementedError, match="kernel_size 4, stride 2, padding 1"):
        _graph("aligned_p2p_unet", nested_levels=2, conv_opts={"dilation": 1})
    with pytest.raises(NotImplementedError, match="running statistics"):
        _graph("p2p_unet", nested_levels=2, sd_edit=lambda sd: [sd.pop(k) for k in list(sd) if "running_" in k or "num_batches" in k])
    with pytest.raises(NotImplementedError, match="8 input channels"):
        _graph("shallow_p2p_unet", nested_levels=1, in_channels=9)
    for precision in ("f16c", "f16ch"):
        with pytest.raises(NotImplementedError, match="f16x3"):
            _graph("inconv_p2p_unet", nested_levels=1, precision=precision)
    with pytest.raises(ValueError):
        unet.AlignedP2pUNet(3, 3, nested_levels=0)                # no skip block: only outconv_unet has that form


def test_conv_cat_validates_its_arguments_without_a_gpu():
    """gdt_net_conv with two inputs: unknown tensor id, transposed / reflect-padded descriptor, channel mismatch with the weight -- ValueError before any HIP call; a refused layer leaves nothing in the graph"""
    net = engine.HipNet(DEV)
    t = net.input(3)
    a = net.conv(t, synth._normal(0, "wa", (64, 3, 1, 1)))
    b = net.conv(t, synth._normal(0, "wb", (128, 3, 1, 1)))
    w = synth._normal(0, "w", (64, 192, 3, 3))
    with pytest.raises(ValueError, match="tensor id"):
        net.conv_cat(a, 99, w, pad=1)
    with pytest.raises(ValueError, match="tensor id"):
        net.conv_cat(-1, b, w, pad=1)
    with pytest.raises(ValueError, match="cin"):
        net.conv_cat(a, b, synth._normal(0, "w", (64, 128, 3, 3)), pad=1)       # 64 + 128 channels against a weight of 128
    with pytest.raises(ValueError, match="cin"):
        net.conv_cat(a, a, w, pad=1)
    out = ctypes.c_int()
    wn = np.ascontiguousarray(w.numpy())
    for bad in (dict(transposed=1), dict(pad_reflect=1)):
        fields = dict(cin=192, cout=64, kh=3, kw=3, stride=1, pad=1, pad_reflect=0, transposed=0, relu=0, out_f32_nchw=0, act=0, bn_eps=1e-5)
        fields.update(bad)
        d = _hip.ConvDesc(**fields)
        with pytest.raises(ValueError):
            _hip.check(net.lib.gdt_net_conv(net.handle, a, b, ctypes.byref(d), ctypes.byref(_hip.ConvWeights(wn.ctypes.data)), -1, ctypes.byref(out)))
    with pytest.raises(ValueError):                                              # BatchNorm vectors come all four or none
        _hip.check(net.lib.gdt_net_conv(net.handle, a, b, ctypes.byref(_hip.ConvDesc(192, 64, 3, 3, 1, 1, 0, 0, 0, 0, 0, 1e-5)),
                                        ctypes.byref(_hip.ConvWeights(wn.ctypes.data, None, wn.ctypes.data)), -1, ctypes.byref(out)))
    ops = net.lib.gdt_net_num_ops(net.handle)
    y = net.conv_cat(a, b, w, pad=1, relu=True)
    assert net.lib.gdt_net_num_ops(net.handle) == ops + 2                        # the copy op of the generic route + the conv
    net.out_slot = net.output_nchw(y)
    assert net.output_shapes(2, 9, 17) == [(2, 64, 9, 17)]
    assert net.conv3x3_cat_launches(2, 9, 17) == 1
    exact = engine.HipNet(DEV, "f16x3")
    te = exact.input(3)
    ye = exact.conv_cat(exact.conv(te, synth._normal(0, "wa", (64, 3, 1, 1))), exact.conv(te, synth._normal(0, "wb", (128, 3, 1, 1))), w, pad=1)
    exact.output_nchw(ye)
    assert exact.conv3x3_cat_launches(2, 9, 17) == 0
    comp = engine.HipNet(DEV, "f16c")
    tc = comp.input(3)
    ac = comp.conv(tc, synth._normal(0, "wa", (64, 3, 1, 1)))
    with pytest.raises(ValueError, match="f16 and f16x3"):
        comp.conv_cat(ac, ac, synth._normal(0, "w", (64, 128, 3, 3)), pad=1)


def _cat_layer(ca, cb, cout):
    net = engine.HipNet(DEV)
    t = net.input(3)
    a = net.conv(t, synth._normal(0, "wa", (ca, 3, 1, 1)))
    b = net.conv(t, synth._normal(0, "wb", (cb, 3, 1, 1)))
    net.output_nchw(net.conv_cat(a, b, synth._normal(0, "w", (cout, ca + cb, 3, 3), 0.01), pad=1))
    return net


def test_conv_cat_routing_rule(monkeypatch):
    """the default route of an eligible layer is the measured one (profiles/p2p_unet_1gpu.json, cat_conv_sweep): the kernel at cout <= 128, where the concatenation
    is no power of two, and where the one-tensor conv has too few patches for its patch kernel; the generic route for wide layers with many patches.
    GDT_CONV3X3_CAT_HALO=2 puts every eligible layer on the kernel, 0 none."""
    monkeypatch.delenv("GDT_CONV3X3_CAT_HALO", raising=False)
    wide, uneven, narrow = _cat_layer(256, 256, 256), _cat_layer(64, 128, 256), _cat_layer(128, 128, 128)
    assert wide.conv3x3_cat_launches(4, 256, 256) == 0 and wide.conv3x3_cat_launches(1, 16, 16) == 1
    assert uneven.conv3x3_cat_launches(4, 256, 256) == 1
    assert narrow.conv3x3_cat_launches(4, 512, 512) == 1 and narrow.conv3x3_cat_launches(1, 1, 1) == 1
    monkeypatch.setenv("GDT_CONV3X3_CAT_HALO", "2")
    assert wide.conv3x3_cat_launches(4, 256, 256) == 1
    monkeypatch.setenv("GDT_CONV3X3_CAT_HALO", "0")
    assert uneven.conv3x3_cat_launches(4, 256, 256) == 0 and wide.conv3x3_cat_launches(1, 16, 16) == 0


def test_conv_cat_knob_is_read_at_every_query(monkeypatch):
    """GDT_CONV3X3_CAT_HALO is a launch knob: 0 -> the generic route, inside one process; it is no plan knob (the layout is the same either way)"""
    net = _graph("aligned_p2p_unet", nested_levels=1)
    monkeypatch.delenv("GDT_CONV3X3_CAT_HALO", raising=False)
    assert net.conv3x3_cat_launches(2, 10, 14) == 1
    ws = net.workspace_bytes(2, 10, 14)
    monkeypatch.setenv("GDT_CONV3X3_CAT_HALO", "0")
    assert net.conv3x3_cat_launches(2, 10, 14) == 0
    assert net.workspace_bytes(2, 10, 14) == ws
    assert "GDT_CONV3X3_CAT_HALO" not in _hip.plan_knobs()


def test_conv_refuses_what_the_routes_do_not_combine():
    """gdt_net_conv, gdt_net_maxpool, gdt_net_pool_head: combinations of descriptor fields no route takes -- ValueError, nothing added to the graph"""
    net = engine.HipNet(DEV)
    t = net.input(3)
    a = net.conv(t, synth._normal(0, "wa", (64, 3, 1, 1)))
    b = net.conv(t, synth._normal(0, "wb", (128, 3, 1, 1)))
    lib, out = net.lib, ctypes.c_int()
    ones = np.ones(64 * 64, np.float32)
    bn = [ones.ctypes.data] * 4

    def conv(in_b, weight_shape, residual=-1, bn=(), **fields):
        w = np.zeros(weight_shape, np.float32)
        transposed = fields.get("transposed", 0)
        d = _hip.ConvDesc(cin=w.shape[0 if transposed else 1], cout=w.shape[1 if transposed else 0], kh=w.shape[2], kw=w.shape[3], bn_eps=1e-5,
                          **dict(dict(stride=1, pad=1), **fields))
        return lib.gdt_net_conv(net.handle, a, in_b, ctypes.byref(d), ctypes.byref(_hip.ConvWeights(w.ctypes.data, None, *bn)), residual, ctypes.byref(out))

    one = ctypes.cast((ctypes.c_float * 1)(3.0), ctypes.c_void_p)
    white = ones.ctypes.data
    refused = {
        "dilation + second input": lambda: conv(b, (64, 192, 3, 3), pad=2, dilation=2),
        "dilation + leaky": lambda: conv(-1, (64, 64, 3, 3), pad=2, dilation=2, leaky=0.2),
        "dilation + BatchNorm": lambda: conv(-1, (64, 64, 3, 3), bn=bn, pad=2, dilation=2),
        "dilation + residual": lambda: conv(-1, (64, 64, 3, 3), residual=a, pad=2, dilation=2),
        "leaky + transposed": lambda: conv(-1, (64, 64, 3, 3), stride=2, transposed=1, leaky=0.2),
        "leaky + transposed 4x4": lambda: conv(-1, (64, 64, 4, 4), stride=2, transposed=1, leaky=0.2),
        "leaky + second input": lambda: conv(b, (64, 192, 3, 3), leaky=0.2),
        "in_relu on a conv": lambda: conv(-1, (64, 64, 3, 3), in_relu=1),
        "in_relu on a conv of two": lambda: conv(b, (64, 192, 3, 3), in_relu=1),
        "in_relu on a transposed 3x3": lambda: conv(-1, (64, 64, 3, 3), stride=2, transposed=1, in_relu=1),
        "residual + second input": lambda: conv(b, (64, 192, 3, 3), residual=a),
        "residual + transposed 4x4 of two": lambda: conv(b, (192, 64, 4, 4), residual=a, stride=2, transposed=1),
        "transposed 4x4: cin is not the inputs' sum": lambda: conv(b, (128, 64, 4, 4), stride=2, transposed=1),
        "ceil pool + padding": lambda: lib.gdt_net_maxpool(net.handle, a, 3, 2, 1, 1, ctypes.byref(out)),
        "attention + final whitening": lambda: lib.gdt_net_pool_head(net.handle, a, ctypes.byref(
            _hip.PoolHeadDesc(2, one, 1, 1e-6, 0, 3, None, None, white, white, 1e-6, 1, 0)), ctypes.byref(out)),
    }
    ops = lib.gdt_net_num_ops(net.handle)
    for what, call in refused.items():
        with pytest.raises(ValueError):
            _hip.check(call())
            pytest.fail("accepted: " + what)
        assert lib.gdt_net_num_ops(net.handle) == ops, what
    # ... and each of them is accepted without the offending field
    assert conv(-1, (64, 64, 3, 3), pad=2, dilation=2) == 0 and conv(-1, (64, 64, 3, 3), leaky=0.2) == 0 and conv(-1, (64, 64, 3, 3), residual=a, bn=bn) == 0
    assert conv(b, (192, 64, 4, 4), stride=2, transposed=1, in_relu=1) == 0 and conv(b, (64, 192, 3, 3)) == 0
    assert lib.gdt_net_maxpool(net.handle, a, 3, 2, 0, 1, ctypes.byref(out)) == 0
    assert lib.gdt_net_pool_head(net.handle, a, ctypes.byref(_hip.PoolHeadDesc(2, one, 1, 1e-6, 0, 3, None, None, None, None, 1e-6, 1, 0)), ctypes.byref(out)) == 0
