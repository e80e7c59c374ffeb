"""``orig_unet`` on the host: the class table and the ``mdir`` alias, the module tree against the reference's key lists and shapes and the CPU forward against the reference's output
(tests/golden/orig_unet.npz), the graph planned without a device -- output shapes, FLOPs against the reference's hook count, the transposed-2 route's plan
counter and its knob, the max-pool behind a tensor with a second reader --, the argument validation of the transposed-2 route of gdt_net_conv, and what the
device path refuses before anything is built.  No GPU."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from gandtr_amd import _hip, engine
from gandtr_amd.components.model.network import unet
from gandtr_amd.tools import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "orig_unet.npz"))
CASES = [i for i in range(int(GOLD["n_cases"])) if str(GOLD["c%d_label" % i]) == "orig_unet"]       # (the fixture also holds the outconv_dynint_unet cases)
OUT_CHANNELS = int(GOLD["out_channels"])
DEV = "cuda:0"        # only recorded; no device call happens before finalize()
KNOB = "GDT_CONVT2X2"


def case(i):
    """(constructor arguments, input shape, weight seed, input seed) of fixture case i"""
    p = "c%d_" % i
    assert str(GOLD[p + "label"]) == "orig_unet"
    cfg = json.loads(str(GOLD[p + "cfg"]))
    wseed, xseed = (int(v) for v in GOLD[p + "seeds"])
    return cfg, tuple(int(v) for v in GOLD[p + "shape"]), wseed, xseed


def _graph(precision="f16", in_channels=3, nested_levels=2, min_channels=64, finalize=False):
    cfg = dict(in_channels=in_channels, out_channels=OUT_CHANNELS, nested_levels=nested_levels, min_channels=min_channels)
    sd = synth.orig_unet_state(0, in_channels=in_channels, out_channels=OUT_CHANNELS, nested_levels=nested_levels, min_channels=min_channels)
    return engine.build_orig_unet(sd, DEV, cfg, precision=precision, finalize=finalize)


def test_class_table_and_alias():
    """the net is reached by its label through ``unet.CLASSES`` (the model registry keeps raising KeyError for it: tests/test_p2p_unet_host.py holds that)"""
    assert unet.CLASSES["orig_unet"] is unet.OrigUNet and unet.OrigUNet.label == "orig_unet"
    m = unet.CLASSES["orig_unet"](in_channels=3, out_channels=2, nested_levels=1)
    assert m.meta == {"in_channels": 3, "out_channels": 2}
    import mdir.components.model.network.unet as alias
    assert alias.OrigUNet is unet.OrigUNet
    import inspect
    params = list(inspect.signature(unet.OrigUNet.__init__).parameters.values())[1:]
    assert [p.name for p in params[:2]] == ["in_channels", "out_channels"]
    assert {p.name: p.default for p in params[2:]} == dict(nested_levels=4, min_channels=64)


@pytest.mark.parametrize("i", CASES)
def test_keys_shapes_meta_and_cpu_forward(i):
    """the module tree gives the reference's state-dict keys in its order, with its shapes (a reference checkpoint loads with strict=True); the CPU forward with the
    synthesised weights is the reference's output within 1e-6 of its range (the same torch ops)"""
    p = "c%d_" % i
    cfg, shape, wseed, xseed = case(i)
    model = unet.CLASSES["orig_unet"](in_channels=shape[1], out_channels=OUT_CHANNELS, **cfg).eval()
    sd = synth.orig_unet_state(wseed, in_channels=shape[1], out_channels=OUT_CHANNELS, **cfg)
    keys = [str(k) for k in GOLD[p + "keys"]]
    assert list(model.state_dict().keys()) == keys
    assert [list(v.shape) + [0] * (4 - v.dim()) for v in model.state_dict().values()] == GOLD[p + "shapes"].tolist()
    assert list(sd.keys()) == keys
    for k in ("outerblock.downconv.conv1.weight", "outerblock.convT.weight", "outerblock.upconv.conv2.bias", "outconv.weight"):
        assert k in keys
    model.load_state_dict(sd, strict=True)
    assert model.meta == {str(k): int(v) for k, v in zip(GOLD[p + "meta_names"], GOLD[p + "meta_values"])}
    ref = torch.from_numpy(GOLD[p + "out"])
    with torch.no_grad():
        y = model(synth.synth_input(xseed, shape, 1.0))
    assert y.shape == ref.shape
    d = float((y - ref).abs().max())
    rng = float(ref.max() - ref.min())
    print("case %d: max|d| = %.3e, range %.3f" % (i, d, rng))
    assert d <= 1e-6 * rng


def test_min_channels_other_than_64():
    """the reference hard-codes outconv = Conv2d(64, out, 1): another min_channels constructs, and its forward fails in torch at outconv; the device path refuses
    it before anything is built"""
    m = unet.OrigUNet(3, 3, nested_levels=1, min_channels=32).eval()
    assert tuple(m.state_dict()["outconv.weight"].shape) == (3, 64, 1, 1) and tuple(m.state_dict()["outerblock.convT.weight"].shape) == (64, 32, 2, 2)
    with torch.no_grad(), pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 8, 8))
    with pytest.raises(NotImplementedError, match="min_channels = 64"):
        _graph(nested_levels=1, min_channels=32)
    with pytest.raises(ValueError):
        unet.OrigUNet(3, 3, nested_levels=0)


@pytest.mark.parametrize("i", CASES)
def test_graph_plans_without_a_device(monkeypatch, i):
    """output of the input's size, at the fixture's size and at the smallest one (2**nested_levels); FLOPs = the reference's hook count; one convt2x2.hip launch
    per transposed conv in f16 (every one of them has cin, cout % 64 == 0), none with the knob at 0, none in f16x3; a size the pools do not divide is refused"""
    monkeypatch.delenv(KNOB, raising=False)
    cfg, shape, _, _ = case(i)
    n, c, h, w = shape
    levels = cfg["nested_levels"]
    for precision in ("f16", "f16x3"):
        net = _graph(precision, in_channels=c, **cfg)
        assert net.output_shapes(n, h, w) == [(n, OUT_CHANNELS, h, w)]
        small = 2 ** levels
        assert net.output_shapes(1, small, 3 * small) == [(1, OUT_CHANNELS, small, 3 * small)]
        assert net.flops(n, h, w) == float(GOLD["c%d_flops" % i])
        assert net.convt2x2_launches(n, h, w) == (levels if precision == "f16" else 0)
        assert net.plan_summary(n, h, w)["conv4x4t_launches"] == 0
        with pytest.raises(ValueError):                               # odd: the two halves of a concatenation differ in size
            net.workspace_bytes(1, small + 1, small)
        if levels > 1:
            with pytest.raises(ValueError):
                net.workspace_bytes(1, small // 2 * 3, small)         # divisible by 2 but not by 2**levels
    net = _graph("f16", in_channels=c, **cfg)
    ws = net.workspace_bytes(n, h, w)
    monkeypatch.setenv(KNOB, "0")
    assert net.convt2x2_launches(n, h, w) == 0
    assert net.workspace_bytes(n, h, w) == ws                         # a launch knob: the same layout either way
    assert KNOB not in _hip.plan_knobs()


def test_pool_behind_a_tensor_with_a_second_reader_stays_its_own_op():
    """x1 = downconv(x) is read by the max-pool AND by the skip (upconv.conv1 reads the pair (x1, x2)): the planner must not let conv2 write the pooled tensor in
    place of x1.  The same conv + pool WITHOUT the second reader is fused (VGG16's stages), so the count below is the second reader's doing."""
    w64 = synth._normal(0, "w", (64, 64, 3, 3), 0.05)

    def chain(skip):
        net = engine.HipNet(DEV)
        t = net.conv(net.input(3), synth._normal(0, "w0", (64, 3, 3, 3), 0.2), pad=1, relu=True)
        x1 = net.conv(t, w64, pad=1, relu=True)
        p = net.conv(net.maxpool(x1, 2, 2, 0), synth._normal(0, "w1", (128, 64, 3, 3), 0.05), pad=1, relu=True)
        if skip:
            x2 = net.conv_transposed2(p, synth._normal(0, "wt", (128, 64, 2, 2), 0.05))
            p = net.conv_cat(x1, x2, synth._normal(0, "w2", (64, 128, 3, 3), 0.05), pad=1, relu=True)
        net.output_nchw(p)
        return net

    for geometry in ((1, 64, 64), (4, 256, 256)):                     # (enough patches for the patch kernels whose epilogue can pool)
        assert chain(False).plan_summary(*geometry)["pools_fused"] == 1
        assert chain(True).plan_summary(*geometry)["pools_fused"] == 0
        assert chain(True).output_shapes(*geometry) == [(geometry[0], 64) + geometry[1:]]
        # the pooled tensor is alive next to x1: the skip's graph needs at least x1 + pool(x1) more scratch than x1 alone
        x1_bytes = geometry[0] * geometry[1] * geometry[2] * 64 * 2
        assert chain(True).workspace_bytes(*geometry) >= x1_bytes + x1_bytes // 4
    for levels in (1, 2, 4):
        net = _graph(nested_levels=levels)
        for geometry in ((1, 32, 48), (1, 64, 64), (4, 256, 256)):
            s = net.plan_summary(*geometry)
            assert s["pools_fused"] == 0 and s["convt2x2_launches"] == levels, s
            assert net.output_shapes(*geometry) == [(geometry[0], OUT_CHANNELS) + geometry[1:]]


def test_transposed2_route_validates_its_arguments_without_a_gpu():
    """gdt_net_conv, transposed-2 route: ValueError before any HIP call, and a refused layer leaves nothing in the graph"""
    net = engine.HipNet(DEV)
    t = net.input(3)
    a = net.conv(t, synth._normal(0, "wa", (128, 3, 1, 1)))
    b = net.conv(t, synth._normal(0, "wb", (64, 3, 1, 1)))
    lib, out = net.lib, ctypes.c_int()
    w = np.zeros((128, 64, 2, 2), np.float32)

    def conv(in_b=-1, residual=-1, weight=w, **fields):
        d = _hip.ConvDesc(cin=weight.shape[0], cout=weight.shape[1], kh=weight.shape[2], kw=weight.shape[3], bn_eps=1e-5, **dict(dict(stride=2, pad=0, transposed=1), **fields))
        return lib.gdt_net_conv(net.handle, a, in_b, ctypes.byref(d), ctypes.byref(_hip.ConvWeights(weight.ctypes.data)), residual, ctypes.byref(out))

    refused = {
        "second input": lambda: conv(in_b=b),
        "residual": lambda: conv(residual=b),
        "external output": lambda: conv(out_f32_nchw=1),
        "reflection padding": lambda: conv(pad_reflect=1),
        "LeakyReLU": lambda: conv(leaky=0.2),
        "ReLU on read": lambda: conv(in_relu=1),
        "dilation": lambda: conv(dilation=2),
        "padding 1 (no such layer)": lambda: conv(pad=1),
        "stride 1 (no such layer)": lambda: conv(stride=1),
        "cin mismatch": lambda: conv(weight=np.zeros((64, 64, 2, 2), np.float32)),
        "cout % 8": lambda: conv(weight=np.zeros((128, 4, 2, 2), np.float32)),
    }
    ops = lib.gdt_net_num_ops(net.handle)
    for what, call in refused.items():
        with pytest.raises(ValueError):
            _hip.check(call())
            pytest.fail("accepted: " + what)
        assert lib.gdt_net_num_ops(net.handle) == ops, what
    with pytest.raises(ValueError, match=r"\[cin\]\[cout\]\[2\]\[2\]"):
        net.conv_transposed2(a, synth._normal(0, "w", (128, 64, 4, 4)))
    y = net.conv_transposed2(a, synth._normal(0, "w", (128, 64, 2, 2)), bias=synth._normal(0, "b", (64,)), relu=True)
    assert lib.gdt_net_num_ops(net.handle) == ops + 1                 # one op, no copy in front
    net.output_nchw(y)
    assert net.output_shapes(2, 5, 7) == [(2, 64, 10, 14)]
    assert net.convt2x2_launches(2, 5, 7) == 1 and net.convt2x2_launches(1, 1, 1) == 1
    assert net.flops(2, 5, 7) == 2.0 * 2 * 5 * 7 * (3 * 128 + 3 * 64 + 128 * 64 * 4)
    comp = engine.HipNet(DEV, "f16c")
    ac = comp.conv(comp.input(3), synth._normal(0, "wa", (128, 3, 1, 1)))
    with pytest.raises(ValueError, match="f16 and f16x3"):
        comp.conv_transposed2(ac, synth._normal(0, "w", (128, 64, 2, 2)))


def test_transposed2_routing_by_channel_counts(monkeypatch):
    """convt2x2.hip takes cin % 64 == 0 and cout % 64 == 0 in f16; everything else runs the four phase launches"""
    monkeypatch.delenv(KNOB, raising=False)

    def layer(cin, cout, precision="f16"):
        net = engine.HipNet(DEV, precision)
        a = net.conv(net.input(3), synth._normal(0, "wa", (cin, 3, 1, 1)))
        net.output_nchw(net.conv_transposed2(a, synth._normal(0, "w", (cin, cout, 2, 2))))
        return net.convt2x2_launches(2, 7, 9)

    assert [layer(128, 64), layer(256, 128), layer(1024, 512), layer(64, 64)] == [1, 1, 1, 1]
    assert [layer(16, 8), layer(128, 24), layer(32, 64)] == [0, 0, 0]
    assert layer(128, 64, "f16x3") == 0


def test_device_path_rejections_that_need_no_device():
    for precision in ("f16c", "f16ch"):
        with pytest.raises(NotImplementedError, match="f16x3"):
            _graph(precision)
    with pytest.raises(NotImplementedError, match="8 input channels"):
        _graph(in_channels=9)
    plan_names = _hip.plan_count_names() + _hip.plan_count_more_names()
    assert _hip.plan_count_more_names() == ("convt2x2_launches",) and len(set(plan_names)) == len(plan_names)
    assert _hip.load().gdt_plan_count_more_name(1) is None and _hip.load().gdt_plan_count_more_name(-1) is None
