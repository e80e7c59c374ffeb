"""RCF on the device (engine.build_rcf; gdt_net_conv_dilated, gdt_net_maxpool_ceil, gdt_net_rcf_head): the new layers one by one against torch
on the tensors they consumed, the whole network against the reference's outputs (tests/golden/rcf.npz) and against the CPU mirror at the
benchmarked geometries, the rcfngan wrapper chain folded into the input pack, determinism, and HED's head unchanged by the shared head-op
plumbing."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_rcf_golden as G                                     # noqa: E402  (seeded inputs, wrapper string; imports no reference code)
from gandtr_amd import engine                                    # noqa: E402
from gandtr_amd.tools import synth                               # noqa: E402

pytestmark = pytest.mark.gpu

# The default (f16) mode: fp16 activations through 13 convs, then a head that sums 13 side dot products of O(100) activations to an O(1-10)
# edge logit.  Measured on an MI355X: pre-sigmoid max|d| / max|ref| 1.42-1.49e-3, sigmoid max|d| 1.4-2.5e-3 -- the same at the geometries where
# conv1_1 reads the fp32 image itself and where the input is packed to fp16 first, so the trunk's fp16 activations, not the input, set it.
# The gates sit above that; the exact mode (f16x3) meets 1e-5 (test_rcf_exact_mode).
PRE_GATE, SIG_GATE = 3e-3, 4e-3


def golden(name="rcf"):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))


def _rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def _model(dev, precision=None):
    from gandtr_amd.components.model.network.rcf import RCF
    m = RCF().eval()
    m.load_state_dict(synth.rcf_state(0))
    m.hip_precision = precision
    return m.to(dev)


@pytest.mark.parametrize("precision,gate", [("f16", 2e-3), ("f16x3", 1e-5)])
@pytest.mark.parametrize("shape", [(2, 31, 31), (2, 23, 37)])
def test_dilated_conv(cuda_device, precision, gate, shape):
    """Conv2d(512, 512, 3, padding=2, dilation=2) + ReLU (RCF conv5_x) against F.conv2d in fp64 on the tensor the layer consumed"""
    n, h, w = shape
    net = engine.HipNet(cuda_device, precision)
    t = net.input(3)
    a = net.conv(t, synth._normal(1, "w0", (512, 3, 1, 1), 0.7), synth._normal(1, "b0", (512,), 0.2), relu=True)
    tap_in = net.output_nchw(a)
    wt, b = synth._normal(1, "w5", (512, 512, 3, 3), (2.0 / (512 * 9)) ** 0.5), synth._normal(1, "b5", (512,), 0.1)
    tap = net.output_nchw(net.conv(a, wt, b, pad=2, relu=True, dilation=2))
    net.finalize()
    assert net.plan_summary(n, h, w)["dilated_special_forms"] == 0
    x = synth.synth_input(3, (n, 3, h, w))
    outs = net.forward(x.to(cuda_device))
    xin, got = outs[tap_in].cpu().double(), outs[tap].cpu()
    wref = wt.half().double() if precision == "f16" else wt.double()
    ref = F.relu(F.conv2d(xin, wref, b.double(), padding=2, dilation=2))
    assert got.shape == ref.shape and _rel(got, ref) < gate
    assert torch.equal(got, net.forward(x.to(cuda_device))[tap].cpu())


@pytest.mark.parametrize("k,s", [(2, 2), (2, 1)])
@pytest.mark.parametrize("shape", [(2, 33, 45), (2, 32, 46), (1, 9, 8)])
def test_ceil_maxpool(cuda_device, k, s, shape):
    """MaxPool2d(k, s, ceil_mode=True) on odd and even maps: bit-identical to torch on the same tensor"""
    n, h, w = shape
    net = engine.HipNet(cuda_device)
    t = net.input(3)
    a = net.conv(t, synth._normal(2, "w", (64, 3, 1, 1), 1.0), relu=False)
    tap_in = net.output_nchw(a)
    tap = net.output_nchw(net.maxpool(a, k, s, ceil=True))
    net.finalize()
    outs = net.forward(synth.synth_input(4, (n, 3, h, w)).to(cuda_device))
    ref = F.max_pool2d(outs[tap_in], k, s, ceil_mode=True)
    assert outs[tap].shape == ref.shape and torch.equal(outs[tap], ref)


@pytest.mark.parametrize("i", [0, 1])
def test_rcf_against_the_reference(cuda_device, i):
    g = golden()
    m = _model(cuda_device)
    x = G.direct_input(i).to(cuda_device)
    with torch.no_grad():
        out, pre = m(x).cpu(), m(x, no_sigmoid=True).cpu()
    assert float((out - torch.from_numpy(g["out%d" % i])).abs().max()) < SIG_GATE
    assert _rel(pre, torch.from_numpy(g["pre%d" % i])) < PRE_GATE


@pytest.mark.parametrize("shape", [(8, 3, 256, 256), (2, 3, 362, 481), (1, 3, 256, 256)])
def test_rcf_against_the_cpu_mirror(cuda_device, shape):
    m = _model(cuda_device)
    cpu = _model("cpu")
    x = synth.synth_input(40, shape, 1.0) * G.DIRECT_SCALE
    with torch.no_grad():
        pre = m(x.to(cuda_device), no_sigmoid=True).cpu()
        out = m(x.to(cuda_device)).cpu()
        ref = cpu(x, no_sigmoid=True)
    assert pre.shape == ref.shape
    assert _rel(pre, ref) < PRE_GATE
    assert float((out - torch.sigmoid(ref)).abs().max()) < SIG_GATE


def test_rcf_exact_mode(cuda_device):
    """Module.hip_precision = "f16x3": the split arithmetic through the generic f16x3 GEMM for the dilated convs"""
    g = golden()
    m = _model(cuda_device, "f16x3")
    with torch.no_grad():
        pre = m(G.direct_input(0).to(cuda_device), no_sigmoid=True).cpu()
    assert _rel(pre, torch.from_numpy(g["pre0"])) < 1e-5


def test_rcf_with_the_rcfngan_wrappers(cuda_device, monkeypatch):
    """the detector of rcfngan.yml through SingleNetwork on the device: all three wrappers fold into the input pack (none runs as a torch op)"""
    from gandtr_amd.learning import network as N
    g = golden()
    params = {"type": "SingleNetwork", "model": {"architecture": "rcf"}, "initialize": False, "runtime": {"wrappers": G.RCFNGAN_WRAPPERS}}
    net = N.initialize_network(params, cuda_device).eval()
    net.model.load_state_dict(synth.rcf_state(0))
    for w in net.wrappers["eval"].wrappers:
        monkeypatch.setattr(w, "preprocess", lambda *a, **k: (_ for _ in ()).throw(AssertionError("wrapper ran as a torch op")))
    with torch.no_grad():
        out = net(G.wrapped_input().to(cuda_device))
    assert out.is_cuda and float((out.cpu() - torch.from_numpy(g["wrapped"])).abs().max()) < SIG_GATE
    keys = [k for k in net.model._hip_cache if isinstance(k, tuple) and k[0] == "rcf"]
    assert keys and keys[0][3] is not None and keys[0][3][0] == (2, 1, 0)


def test_rcf_deterministic(cuda_device):
    net = engine.build_rcf(synth.rcf_state(0), cuda_device)
    x = (synth.synth_input(41, (2, 3, 130, 97), 1.0) * G.DIRECT_SCALE).to(cuda_device)
    a = net.forward(x)[net.out_slot].clone()
    b = net.forward(x)[net.out_slot]
    assert torch.equal(a, b)


def test_hed_head_unchanged(cuda_device):
    """HED's output in the default mode, bit for bit what the library computed before the head ops shared their plumbing with RCF
    (tests/golden/hed_device_f16.npz: recorded on an MI355X with the previous library)"""
    g = golden("hed_device_f16")
    net = engine.build_hed(synth.hed_state(0), cuda_device)
    x = synth.synth_input(8, (2, 3, 64, 96), 1.0).to(cuda_device)
    out = net.forward(x)[net.out_slot].cpu().numpy()
    assert np.array_equal(out, g["out"])
