"""GPU parity of conv3x3_halo_c16.hip where a workgroup walks MORE than one tile: a 3x3 256 -> 256 conv with reflect padding on 20 x 64 x 64 is
320 patches of 16 x 16 for the chip's 256 workgroups, so 64 of them take a second tile -- the halo of the next tile's first chunk is staged
during the last chunk of the current one, from the other slot of the normalisation table (`to_next`).  The layer tests of test_hip_f16c.py stop
at 256 patches, one tile per workgroup.

The forms are built as in test_hip_f16c.py::test_halo_c_conv3x3 and held to the same bounds: 2e-4 of an fp64 evaluation of the layer on the
same fp32 inputs, 3e-4 for the InstanceNorm that follows, 1e-5 for the written-back normalised tensor (plain fp32).  The kernel sums in a
fixed order, so a second forward is bitwise the first."""
import pytest
import torch
import torch.nn.functional as F

from gandtr_amd.engine import HipNet
from gandtr_amd.tools import synth

pytestmark = pytest.mark.gpu

N, C = 20, 256
# form -> (producer's InstanceNorm folded, + residual folded, normalised tensor written back, residual added in the epilogue)
FORMS = {"plain_epilogue_residual": (False, False, False, True), "norm": (True, False, False, False), "norm_writeback": (True, False, True, False),
         "norm_residual_writeback": (True, True, True, False)}
_cache = {}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _g(name, shape, std):
    return synth._normal(0, name, shape, std)


def _reference(norm, res):
    """fp64 on the host, once per distinct conv input: (the conv's input, the conv 256 -> 256 of it without the epilogue residual, the 1x1 stem output)"""
    if "x" not in _cache:
        _cache["x"] = synth.synth_input(1, (N, 3, 64, 64))
        _cache["a0"] = F.conv2d(_cache["x"].double(), _g("w0", (C, 3, 1, 1), 0.7).double())
    a0 = _cache["a0"]
    if (norm, res) not in _cache:
        a = a0
        if norm:
            a = F.instance_norm(a0, eps=1e-5)
            a = a + F.conv2d(a0, _g("w1", (C, C, 1, 1), 0.06).double()) if res else F.relu(a)
        y = F.conv2d(F.pad(a, (1,) * 4, mode="reflect"), _g("w", (C, C, 3, 3), 0.05).double(), _g("b", (C,), 0.2).double())
        _cache[(norm, res)] = (a, y)
    return _cache[(norm, res)] + (a0,)


@pytest.mark.parametrize("form", list(FORMS))
def test_c16_second_tile(cuda_device, form):
    norm, res, wb, epi_res = FORMS[form]
    net = HipNet(cuda_device, "f16c")
    t = net.input(3)
    t0 = net.conv(t, _g("w0", (C, 3, 1, 1), 0.7))
    t = t0
    if norm:
        r = net.conv(t0, _g("w1", (C, C, 1, 1), 0.06)) if res else -1
        t = net.instance_norm(t0, relu=not res, residual=r)
    out = net.conv(t, _g("w", (C, C, 3, 3), 0.05), _g("b", (C,), 0.2), pad=1, reflect=True, residual=t0 if epi_res else -1)
    o2 = net.instance_norm(out, relu=True)
    taps = [net.output_nchw(out), net.output_nchw(o2)] + ([net.output_nchw(t)] if wb else [])
    net.finalize()
    a, y, a0 = _reference(norm, res)
    x = _cache["x"].to(cuda_device)
    net.set_profiling(True)
    outs = net.forward(x)
    torch.cuda.synchronize()
    ran = [v for k, v, ms, fl in net.profile() if k == 1]
    first = [outs[k].clone() for k in taps]
    outs = net.forward(x)
    torch.cuda.synchronize()
    second = [outs[k] for k in taps]
    ref = y + a0 if epi_res else y
    figures = {"out": _rel(first[0].double().cpu(), ref), "norm_after": _rel(first[1].double().cpu(), F.relu(F.instance_norm(ref, eps=1e-5)))}
    if wb:
        figures["writeback"] = _rel(first[2].double().cpu(), a)
    print(form, "variants", sorted(set(ran)), figures)
    assert 971256 in ran, ran                  # conv3x3_halo_c16.hip ran the layer
    assert figures["out"] < 2e-4
    assert figures["norm_after"] < 3e-4
    if wb:
        assert figures["writeback"] < 1e-5
    for p, q in zip(first, second):
        assert torch.equal(p, q)
