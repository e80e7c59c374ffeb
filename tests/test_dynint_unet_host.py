"""``outconv_dynint_unet`` on the host: the class table, the module tree against the reference's key lists and shapes and the CPU forward against the reference's
output (the dynint cases of tests/golden/orig_unet.npz), the graph planned without a device -- output shapes at even, odd and minimal sizes, FLOPs against the
reference's hook count, sizes whose innermost map would be empty --, the argument validation of gdt_net_resize, and what the device path refuses before
anything is built.  No GPU."""
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
CASES = [i for i in range(int(GOLD["n_cases"])) if str(GOLD["c%d_label" % i]) == "outconv_dynint_unet"]
OUT_CHANNELS = int(GOLD["out_channels"])
DEV = "cuda:0"        # only recorded; no device call happens before finalize()


def case(i):
    """(constructor arguments, input shape, weight seed, input seed) of fixture case i"""
    p = "c%d_" % i
    wseed, xseed = (int(v) for v in GOLD[p + "seeds"])
    return json.loads(str(GOLD[p + "cfg"])), tuple(int(v) for v in GOLD[p + "shape"]), wseed, xseed


def state(seed, in_channels, cfg):
    return synth.dynint_unet_state(seed, in_channels=in_channels, out_channels=OUT_CHANNELS, **{k: v for k, v in cfg.items() if k != "upsample"})


def _graph(precision="f16", in_channels=3, finalize=False, **cfg):
    model = unet.OutconvP2pUNetDynamicInterpolate(in_channels, OUT_CHANNELS, **cfg)
    weights = {k: v for k, v in cfg.items() if k in ("nested_levels", "outconv_channels", "outconv_kernel", "batchnorm")}
    return engine.build_dynint_unet(state(0, in_channels, weights), DEV, model._cfg, precision=precision, finalize=finalize)


def test_class_table_and_constructor():
    """the net is reached by its label through ``unet.CLASSES`` (the model registry keeps raising KeyError for it: tests/test_p2p_unet_host.py holds that)"""
    assert unet.CLASSES["outconv_dynint_unet"] is unet.OutconvP2pUNetDynamicInterpolate and unet.OutconvP2pUNetDynamicInterpolate.label == "outconv_dynint_unet"
    m = unet.CLASSES["outconv_dynint_unet"](in_channels=1, out_channels=2, nested_levels=1)
    assert m.meta == {"in_channels": 1, "out_channels": 2}
    import inspect
    params = list(inspect.signature(unet.OutconvP2pUNetDynamicInterpolate.__init__).parameters.values())[1:]
    assert [p.name for p in params[:2]] == ["in_channels", "out_channels"]
    assert {p.name: p.default for p in params[2:]} == dict(conv_opts=None, upconv_opts=None, nested_levels=7, upsample="bilinear", outconv_channels=32,
                                                           outconv_kernel=3, dropout=False, batchnorm=False)
    with pytest.raises(AssertionError):
        unet.OutconvP2pUNetDynamicInterpolate(3, 3, outconv_kernel=4)


@pytest.mark.parametrize("i", CASES)
def test_keys_shapes_meta_and_cpu_forward(i):
    """the module tree gives the reference's state-dict keys in its order, with its shapes; the CPU forward with the synthesised weights is the reference's
    output within 1e-6 of its range (the same torch ops)"""
    p = "c%d_" % i
    cfg, shape, wseed, xseed = case(i)
    model = unet.CLASSES["outconv_dynint_unet"](in_channels=shape[1], out_channels=OUT_CHANNELS, **cfg).eval()
    sd = state(wseed, shape[1], cfg)
    keys = [str(k) for k in GOLD[p + "keys"]]
    assert list(model.state_dict().keys()) == keys
    assert [list(v.shape) + [0] * (4 - v.dim()) for v in model.state_dict().values()] == GOLD[p + "shapes"].tolist()
    assert list(sd.keys()) == keys
    assert "up.0.weight" in keys and ("down.2.down.0.weight" in keys)
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


@pytest.mark.parametrize("i", CASES)
def test_graph_plans_without_a_device(i):
    """output of the input's size at the fixture's size (odd sizes among them), at even ones and at the smallest one (2**(nested_levels + 1): an innermost map
    of one pixel); FLOPs = the reference's hook count (every map is floor(H / 2) of the one above); a size whose innermost map would be empty is refused"""
    cfg, shape, _, _ = case(i)
    n, c, h, w = shape
    small = 2 ** (cfg["nested_levels"] + 1)
    for precision in ("f16", "f16x3"):
        net = _graph(precision, in_channels=c, **cfg)
        assert net.flops(n, h, w) == float(GOLD["c%d_flops" % i])
        for geometry in ((n, h, w), (1, 64, 96), (1, small, small + 1), (2, small + 5, 3 * small + 1)):
            assert net.output_shapes(*geometry) == [(geometry[0], OUT_CHANNELS) + geometry[1:]]
            assert net.workspace_bytes(*geometry) > 0
        with pytest.raises(ValueError, match="empty"):
            net.workspace_bytes(1, small - 1, 4 * small)
        assert net.plan_summary(n, h, w)["convt2x2_launches"] == 0


def test_resize_validates_its_arguments_without_a_gpu():
    """gdt_net_resize: unknown tensor ids and modes -- ValueError before any HIP call, nothing added to the graph; the output has in_tensor's channels and
    like_tensor's size, per geometry"""
    net = engine.HipNet(DEV)
    t = net.input(3)
    like = net.conv(t, synth._normal(0, "wa", (16, 3, 1, 1)))
    small = net.conv(like, synth._normal(0, "wb", (64, 16, 4, 4)), stride=2, pad=1)
    lib, out = net.lib, ctypes.c_int()
    ops = lib.gdt_net_num_ops(net.handle)
    for args in ((99, like, 0), (small, 99, 0), (-1, like, 0), (small, -1, 0), (small, like, 2), (small, like, -1)):
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_net_resize(net.handle, *args, ctypes.byref(out)))
        assert lib.gdt_net_num_ops(net.handle) == ops
    with pytest.raises(NotImplementedError, match="bilinear"):
        net.resize(small, like, "bicubic")
    r = net.resize(small, like, "bilinear")
    assert lib.gdt_net_num_ops(net.handle) == ops + 1
    net.output_nchw(r)
    net.output_nchw(net.resize(r, small, "nearest"))                  # down again, to the small map's size
    assert net.output_shapes(2, 11, 15) == [(2, 64, 11, 15), (2, 64, 5, 7)]
    assert net.output_shapes(1, 2, 3) == [(1, 64, 2, 3), (1, 64, 1, 1)]
    assert net.flops(2, 11, 15) == 2.0 * 2 * (11 * 15 * 3 * 16 + 5 * 7 * 16 * 64 * 16)      # a resize counts no conv FLOPs


def test_device_path_rejections_that_need_no_device():
    with pytest.raises(NotImplementedError, match="upsample = 'bicubic'"):
        _graph(nested_levels=1, upsample="bicubic")
    with pytest.raises(NotImplementedError, match="kernel_size 4, stride 2, padding 1"):
        _graph(nested_levels=1, conv_opts={"kernel_size": 2, "padding": 0})
    with pytest.raises(NotImplementedError, match="kernel_size 3, stride 1, padding 1"):
        _graph(nested_levels=1, upconv_opts={"kernel_size": 1, "padding": 0})
    with pytest.raises(NotImplementedError, match="8 input channels"):
        _graph(nested_levels=1, in_channels=9)
    for precision in ("f16c", "f16ch"):
        with pytest.raises(NotImplementedError, match="f16x3"):
            _graph(precision, nested_levels=1)
    # ... all of which are plain torch on the CPU
    m = unet.OutconvP2pUNetDynamicInterpolate(3, 2, conv_opts={"kernel_size": 2, "padding": 0}, upconv_opts={"kernel_size": 1, "padding": 0}, nested_levels=2,
                                              upsample="bicubic", dropout=0.25, batchnorm=True).eval()
    with torch.no_grad():
        assert tuple(m(torch.zeros(1, 3, 9, 13)).shape) == (1, 2, 9, 13)
    assert any(isinstance(mod, torch.nn.Dropout) and mod.p == 0.25 for mod in m.modules())
