"""RCF (mdir/components/model/network/rcf.py) on the host: registry, state_dict layout, the CPU forward against the reference's own outputs
(tests/golden/rcf.npz, made by tests/golden/make_rcf_golden.py), argument validation of the three C entries it needs and the planner's
decisions for its graph.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_rcf_golden as G                                     # noqa: E402  (seeded inputs, wrapper string; imports no reference code)
from gandtr_amd import engine                                    # noqa: E402
from gandtr_amd.tools import synth                               # noqa: E402

DEV = "cuda:0"        # only recorded; no device call happens before finalize()


def golden():
    return np.load(os.path.join(HERE, "golden", "rcf.npz"))


def _model():
    import mdir                                                  # noqa: F401
    from mdir.components.model.network import MODEL_LABELS
    m = MODEL_LABELS["rcf"]().eval()
    m.load_state_dict(synth.rcf_state(0))
    return m


def test_registered_and_aliased():
    import mdir                                                  # noqa: F401
    from mdir.components.model.network import MODEL_LABELS, rcf
    from gandtr_amd.components.model.network import rcf as mirror
    assert MODEL_LABELS["rcf"] is mirror.RCF and rcf is mirror
    assert mirror.RCF.meta == {"in_channels": 3, "out_channels": 1} and mirror.RCF.accepts_input_transform


def test_state_dict_layout_and_pretrained(tmp_path):
    g = golden()
    from gandtr_amd.components.model.network.rcf import RCF
    m = RCF()
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]] and len(sd) == 64
    for (k, v), shp in zip(sd.items(), g["shapes"]):
        assert list(v.shape) == [int(s) for s in shp[:v.dim()]] and all(int(s) == 0 for s in shp[v.dim():]), k
    assert sorted(dict(m.named_buffers())) == ["weight_deconv%d" % k for k in range(2, 6)]        # non-persistent: not state
    path = tmp_path / "rcf.pth"
    torch.save(synth.rcf_state(0), str(path))
    loaded = RCF(pretrained=str(path))
    for k, v in synth.rcf_state(0).items():
        assert torch.equal(loaded.state_dict()[k], v), k


@pytest.mark.parametrize("i", [0, 1])
def test_cpu_forward_matches_reference(i):
    g = golden()
    m = _model()
    x = G.direct_input(i)
    with torch.no_grad():
        out, pre = m(x), m(x, no_sigmoid=True, features=True, interpolate=True)
    assert out.shape == (G.GEOMETRIES[i][0], 1) + G.GEOMETRIES[i][2:]
    assert float((out - torch.from_numpy(g["out%d" % i])).abs().max()) < 1e-5
    assert float((pre - torch.from_numpy(g["pre%d" % i])).abs().max()) < 1e-5


def test_cpu_forward_through_the_rcfngan_wrappers():
    g = golden()
    from gandtr_amd.learning import network as N
    params = {"type": "SingleNetwork", "model": {"architecture": "rcf"}, "initialize": False, "runtime": {"wrappers": G.RCFNGAN_WRAPPERS}}
    net = N.initialize_network(params, "cpu").eval()
    net.model.load_state_dict(synth.rcf_state(0))
    with torch.no_grad():
        out = net(G.wrapped_input())
    assert float((out - torch.from_numpy(g["wrapped"])).abs().max()) < 1e-5


def test_too_small_input_raises():
    """8 x 8: pool4 leaves an empty map, the reference raises; the mirror and the HIP planner do too"""
    m = _model()
    with pytest.raises((RuntimeError, AssertionError)):
        with torch.no_grad():
            m(torch.zeros(1, 3, 8, 8))
    net = engine.build_rcf(synth.rcf_state(0), DEV, finalize=False)
    with pytest.raises(ValueError):
        net.output_shapes(1, 8, 8)
    assert net.output_shapes(1, 9, 9) == [(1, 1, 9, 9)] and net.output_shapes(2, 45, 61) == [(2, 1, 45, 61)]


def test_c_entries_validate_arguments_without_gpu():
    from gandtr_amd import _hip
    lib = _hip.load()
    h = ctypes.c_void_p()
    _hip.check(lib.gdt_net_create(ctypes.byref(h)))
    try:
        out = ctypes.c_int()
        _hip.check(lib.gdt_net_input(h, 3, None, None, None, ctypes.byref(out)))
        x = out.value
        w = np.zeros((64, 3, 3, 3), np.float32)
        d = _hip.ConvDesc(3, 64, 3, 3, 1, 2, 0, 0, 1, 0, 0, 1e-5, dilation=2)
        wts = _hip.ConvWeights(w.ctypes.data_as(ctypes.c_void_p))

        def conv(in_tensor, desc):
            return lib.gdt_net_conv(h, in_tensor, -1, ctypes.byref(desc), ctypes.byref(wts), -1, ctypes.byref(out))
        with pytest.raises(ValueError):
            _hip.check(conv(99, d))                                                                             # unknown tensor id
        with pytest.raises(ValueError):
            _hip.check(conv(x, _hip.ConvDesc(3, 64, 3, 3, 1, 2, 0, 0, 1, 0, 0, 1e-5, dilation=0)))              # dilation < 1
        with pytest.raises(ValueError):
            _hip.check(conv(x, _hip.ConvDesc(3, 64, 3, 3, 2, 1, 0, 1, 0, 0, 0, 1e-5, dilation=2)))              # transposed + dilation
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_net_maxpool(h, 99, 2, 2, 0, 1, ctypes.byref(out)))                               # ceil mode: unknown tensor id
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_net_maxpool(h, x, 2, 0, 0, 1, ctypes.byref(out)))                                # ceil mode: stride 0
        _hip.check(conv(x, d))
        f = out.value
        side = np.zeros(64, np.float32)
        sw = (ctypes.c_void_p * 13)(*[side.ctypes.data] * 13)
        b5 = (ctypes.c_float * 5)(*[0.0] * 5)
        good = [0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4]

        def head(feats, stages):
            return lib.gdt_net_rcf_head(h, (ctypes.c_int * 13)(*feats), (ctypes.c_int * 13)(*stages), sw, b5, b5, 0.0, 1, ctypes.byref(out))
        with pytest.raises(ValueError):
            _hip.check(head([f] * 12 + [99], good))                                                             # unknown tensor id
        with pytest.raises(ValueError):
            _hip.check(head([f] * 13, [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 4]))                                 # 4 features in one stage
        with pytest.raises(ValueError):
            _hip.check(head([f] * 13, [0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 3, 3, 3]))                                 # stage 5 missing
        with pytest.raises(ValueError):
            _hip.check(head([f] * 13, [0, 1, 0, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4]))                                 # stages out of order
        with pytest.raises(ValueError):
            _hip.check(head([f] * 13, [0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 5]))                                 # stage 6 does not exist
        _hip.check(head([f] * 13, good))
    finally:
        lib.gdt_net_destroy(h)
    with pytest.raises(ValueError):
        engine.build_rcf(synth.rcf_state(0), DEV, finalize=False).rcf_head([1] * 12, [0] * 12, [side] * 12, [0.0] * 5, [0.0] * 5, 0.0)   # 12 features


def test_conv_desc_defaults_to_no_dilation():
    """the twelve-field construction means "no dilation"; an explicit dilation of 0 reaches the library, which refuses it"""
    from gandtr_amd import _hip
    d = _hip.ConvDesc(3, 64, 3, 3, 1, 1, 0, 0, 1, 0, 0, 1e-5)
    assert d.dilation == 1 and d.leaky == 0.0 and d.in_relu == 0
    assert _hip.ConvDesc(3, 64, 3, 3, 1, 1, 0, 0, 1, 0, 0, 1e-5, dilation=0).dilation == 0
    net = engine.HipNet(DEV)
    x = net.input(3)
    ops = net.lib.gdt_net_num_ops(net.handle)
    with pytest.raises(ValueError):
        net.conv(x, torch.zeros(64, 3, 3, 3), pad=1, dilation=0)
    assert net.lib.gdt_net_num_ops(net.handle) == ops
    net.conv(x, torch.zeros(64, 3, 3, 3), pad=1)


def test_planner_keeps_dilated_convs_and_side_tensors_plain():
    """Every dilated conv runs on a generic implicit-GEMM kernel (no patch kernel stages a 2-pixel halo), and no pool is fused into its producer:
    every pre-pool tensor (conv1_2, conv2_2, conv3_3, conv4_3) also feeds the side output; HED's 4 pools are not fused for the same reason."""
    net = engine.build_rcf(synth.rcf_state(0), DEV, finalize=False)
    for geo in ((2, 64, 96), (1, 45, 61), (64, 256, 256), (8, 362, 481)):
        p = net.plan_summary(*geo)
        assert p["dilated_convs"] == 3 and p["dilated_special_forms"] == 0, (geo, p)
        assert p["pools_fused"] == 0 and p["conv_launches"] == 13, (geo, p)
    assert net.plan_summary(64, 256, 256)["direct_stem"] == 1                  # conv1_1 reads the fp32 image itself
    assert net.flops(1, 256, 256) / 1e9 == pytest.approx(50.11, abs=0.01)      # conv1 5.06 + conv2 7.25 + conv3 12.08 + conv4 12.08 + conv5 13.60 + head
    assert net.output_shapes(8, 362, 481) == [(8, 1, 362, 481)]
    for prec in ("f16x3", "f16c"):
        p = engine.build_rcf(synth.rcf_state(0), DEV, precision=prec, finalize=False).plan_summary(2, 64, 96)
        assert p["dilated_convs"] == 3 and p["dilated_special_forms"] == 0, (prec, p)


def test_ceil_pool_shapes_follow_torch():
    """gdt_net_maxpool with ceil_mode: torch's ceil_mode output size, odd and even, stride 2 and 1; floor mode unchanged"""
    for k, s in ((2, 2), (2, 1), (3, 2)):
        for hw in ((7, 10), (8, 9), (3, 4), (33, 31)):
            net = engine.HipNet(DEV)
            t = net.input(3)
            a = net.conv(t, torch.zeros(8, 3, 1, 1))
            net.output_nchw(net.maxpool(a, k, s, ceil=True))
            net.output_nchw(net.maxpool(a, k, s))
            ref_c = torch.nn.functional.max_pool2d(torch.zeros(1, 8, *hw), k, s, ceil_mode=True).shape
            ref_f = torch.nn.functional.max_pool2d(torch.zeros(1, 8, *hw), k, s).shape
            assert net.output_shapes(1, *hw) == [tuple(ref_c), tuple(ref_f)], (k, s, hw)
