"""The descriptor heads on the device: the one-pass region pooling kernel on its own (through the C ABI), every net case of
tests/golden/descriptor_heads.npz against the reference's descriptors, one real geometry against the CPU mirror, the concurrent / multi-scale
paths, and that the plain GeM embedder is planned as before."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_descriptor_heads_golden as G                        # noqa: E402  (seeded inputs, case lists; imports no reference code)
from gandtr_amd import _hip, engine                             # noqa: E402
from gandtr_amd.components.data import wrapper                  # noqa: E402
from gandtr_amd.components.model.network import cirnet          # noqa: E402
from gandtr_amd.components.model.network._hipbacked import ScaledInput   # noqa: E402
from gandtr_amd.tools import synth                              # noqa: E402

KINDS = {"mac": 0, "spoc": 1, "gem3": 2, "gem237": 2, "gemmp": 3}
# the descriptor gates of the project (tests/test_hip_golden.py): |d - ref|_inf < 1e-3, cosine > 0.9999
GATE_ABS, GATE_COS = 1e-3, 0.9999
# f16x3 (fp32-class convs): the worst error measured over the net cases on an MI355X, asserted at four times the measurement (run-to-run and
# box-to-box slack on an error that is rounding noise)
X3_MEASURED_ABS = 1.937e-07                                      # vgg16-mac; the other ten cases 3.7e-08 .. 1.1e-07
X3_MEASURED_COS_DEFECT = 3.466e-13                               # 1 - cosine (evaluated in float64), the same case


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "descriptor_heads.npz"))


def pool_regions(x_nhwc, kind, p, p_channels, levels, eps=1e-6):
    """gdt_pool_regions on an N x H x W x D device tensor (fp16 or fp32) -> N x R x D"""
    lib = _hip.load()
    n, h, w, d = x_nhwc.shape
    cnt = ctypes.c_int()
    _hip.check(lib.gdt_rpool_regions(h, w, levels, None, 0, ctypes.byref(cnt)))
    out = torch.full((n, cnt.value, d), float("nan"), dtype=torch.float32, device=x_nhwc.device)
    with torch.cuda.device(x_nhwc.device):
        _hip.check(lib.gdt_pool_regions(x_nhwc.data_ptr(), int(x_nhwc.dtype == torch.float32), n, h, w, d, kind, float(p),
                                        None if p_channels is None else p_channels.data_ptr(), eps, levels, out.data_ptr(),
                                        torch.cuda.current_stream(x_nhwc.device).cuda_stream))
    torch.cuda.synchronize(x_nhwc.device)
    return out


def host_regions(x, pool, levels):
    """the mirror's roipool (N x R x D), or the pooling of the whole map alone for levels = 0"""
    if levels == 0:
        return pool(x).flatten(1).unsqueeze(1)
    return cirnet.roipool(x, pool, levels).flatten(2)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("si", range(len(G.LAYER_SIZES)), ids=["%dx%d" % s for s in G.LAYER_SIZES])
def test_region_pooling_kernel(cuda_device, si, dtype):
    """max: bit-exact against the mirror on the same (rounded) input; mean / GeM kinds: within the 1e-5 absolute that test_gem_l2n_golden
    (tests/test_hip_f16c.py) asks of the plain GeM op, against a float64 evaluation of the same input; two runs give the same bits.  Four of the
    six sizes are ragged (a width that is no multiple of the eight pixels a lane loads at once, down to a 1 x 3 map)."""
    p_mp = G.layer_params()[0]
    p_dev = p_mp.to(cuda_device)
    for kind in G.LAYER_KINDS:
        x = G.layer_map(si, kind).to(dtype).float()                         # what the kernel sees, as fp32 on the host
        xd = x.permute(0, 2, 3, 1).contiguous().to(cuda_device, dtype)
        for levels in (0, 3):
            got = pool_regions(xd, 0, 1.0, None, levels)
            assert torch.equal(got.cpu(), host_regions(x, cirnet.mac, levels)), ("mac", kind, levels)
            x64 = x.double()
            cases = {"spoc": (cirnet.spoc, 1.0, None), "gem3": (lambda t: cirnet.gem(t, 3.0), 3.0, None),
                     "gem237": (lambda t: cirnet.gem(t, 2.37), 2.37, None),
                     "gemmp": (lambda t: cirnet.gem(t, p_mp.double().view(1, -1, 1, 1)), 1.0, p_dev)}
            for name, (pool, p, pch) in cases.items():
                got = pool_regions(xd, KINDS[name], p, pch, levels)
                ref = host_regions(x64, pool, levels)
                err = float((got.cpu().double() - ref).abs().max())
                print("%s %s %s levels %d: max|d| %.3e" % (G.LAYER_SIZES[si], kind, name, levels, err))
                assert got.shape == ref.shape and err <= 1e-5, (name, kind, levels, err)
                assert torch.equal(got, pool_regions(xd, KINDS[name], p, pch, levels)), ("not reproducible", name, kind, levels)


@pytest.mark.gpu
def test_region_pooling_bad_arguments(cuda_device):
    x = torch.zeros((1, 4, 4, 64), dtype=torch.float32, device=cuda_device)
    with pytest.raises(ValueError):
        pool_regions(x, 7, 1.0, None, 0)                                    # no such kind
    with pytest.raises(ValueError):
        pool_regions(x, 3, 1.0, None, 0)                                    # per-channel GeM without its exponents
    with pytest.raises(ValueError):
        pool_regions(x[..., :32].contiguous(), 0, 1.0, None, 0)             # channels % 64


def device_net(case, seed, device, precision=None):
    net = G.build_net(cirnet.init_cirnet, case, seed)
    net.hip_precision = precision
    return net.to(device)


def errors(got, ref):
    got, ref = got.detach().cpu().double(), torch.as_tensor(np.asarray(ref)).double()
    return float((got - ref).abs().max()), float(torch.nn.functional.cosine_similarity(got, ref, dim=0).min())


@pytest.mark.gpu
@pytest.mark.parametrize("case", G.NET_CASES, ids=G.case_name)
def test_nets_f16_against_the_reference(cuda_device, golden, case):
    name = G.case_name(case)
    net = device_net(case, int(golden["net_%s_seed" % name]), cuda_device)
    with torch.no_grad():
        out = net(G.net_input().to(cuda_device))
    err, cos = errors(out, golden["net_%s_out" % name])
    print("%s f16: max|d| %.3e  min cosine %.7f" % (name, err, cos))
    assert out.shape == (net.meta["outputdim"], G.NET_INPUT[0])
    assert err < GATE_ABS and cos > GATE_COS, (name, err, cos)


@pytest.mark.gpu
def test_nets_f16x3_against_the_reference(cuda_device, golden):
    worst_err, worst_cos = 0.0, 1.0
    for case in G.NET_CASES:
        name = G.case_name(case)
        net = device_net(case, int(golden["net_%s_seed" % name]), cuda_device, "f16x3")
        with torch.no_grad():
            out = net(G.net_input().to(cuda_device))
        err, cos = errors(out, golden["net_%s_out" % name])
        print("%s f16x3: max|d| %.3e  1 - min cosine %.3e" % (name, err, 1.0 - cos))
        worst_err, worst_cos = max(worst_err, err), min(worst_cos, cos)
    print("f16x3 worst: max|d| %.3e  1 - min cosine %.3e" % (worst_err, 1.0 - worst_cos))
    assert worst_err <= 4 * X3_MEASURED_ABS and 1.0 - worst_cos <= 4 * X3_MEASURED_COS_DEFECT, (worst_err, 1.0 - worst_cos)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("resnet101", "gem", False, True, True), ("vgg16", "mac", False, True, False)], ids=G.case_name)
def test_real_geometry_against_the_cpu_mirror(cuda_device, case):
    """2 images of 1024 x 768: a 64 x 48 (VGG) / 32 x 24 (ResNet) map, 21 regions"""
    net = G.build_net(cirnet.init_cirnet, case, 1000)
    x = synth.synth_input(330, (2, 3, 1024, 768))
    with torch.no_grad():
        ref = net(x)
        out = net.to(cuda_device)(x.to(cuda_device))
    err, cos = errors(out, ref)
    print("%s 2 x 1024 x 768 f16: max|d| %.3e  min cosine %.7f" % (G.case_name(case), err, cos))
    assert err < GATE_ABS and cos > GATE_COS, (err, cos)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("vgg16", "gem", False, True, True), ("vgg16", "rmac", False, False, False), ("resnet101", "gemmp", False, False, True)],
                         ids=G.case_name)
def test_forward_many_and_multiscale_with_a_head(cuda_device, case, monkeypatch):
    net = device_net(case, 1000, cuda_device)
    x = synth.synth_input(331, (2, 3, 160, 224)).to(cuda_device)
    ms = wrapper.CirMultiscaleAggregation("ms", cuda_device)
    levels, _ = ms.preprocess(x, net)
    assert all(isinstance(l, ScaledInput) for l in levels) and len(levels) == 3
    with torch.no_grad():
        many = net.forward_many(levels)
        single = [net(l) for l in levels]
    torch.cuda.synchronize(cuda_device)
    for a, b in zip(many, single):
        assert torch.equal(a, b)
    seen = []
    real = wrapper.CirMultiscaleAggregation.aggregate_tensor
    monkeypatch.setattr(wrapper.CirMultiscaleAggregation, "aggregate_tensor", staticmethod(lambda t, ns, dim, msp: (seen.append(msp), real(t, ns, dim, msp))[1]))
    agg = ms.postprocess(many, net, False)
    assert seen == [1] and agg.shape == (net.meta["outputdim"], 2)
    plain = device_net(("vgg16", "gem", False, False, False), 1000, cuda_device)
    plain.pool.p.data.fill_(2.5)
    with torch.no_grad():
        ms.postprocess(plain.forward_many(levels), plain, False)
    assert seen == [1, 2.5]


@pytest.mark.gpu
def test_swapping_the_head_rebuilds_the_device_net(cuda_device):
    net = device_net(("vgg16", "gem", False, False, True), 1000, cuda_device)
    x = synth.synth_input(332, (1, 3, 96, 128)).to(cuda_device)
    with torch.no_grad():
        a = net(x)
        net.whiten = None
        b = net(x)                                                          # the plain GeM op again
        net.pool = cirnet.MAC()
        c = net(x)
    assert not torch.equal(a, b) and not torch.equal(b, c)
    ref = G.build_net(cirnet.init_cirnet, ("vgg16", "mac", False, False, False), 1000)
    with torch.no_grad():
        err, cos = errors(c, ref(x.cpu()))
    assert err < GATE_ABS and cos > GATE_COS


def host_graph():
    """a layer graph without a device: the builder calls and the planner are host code"""
    net = engine.HipNet.__new__(engine.HipNet)
    net.lib, net.precision, net.handle = _hip.load(), "f16", ctypes.c_void_p()
    _hip.check(net.lib.gdt_net_create(ctypes.byref(net.handle)))
    return net


def test_head_launches_do_not_depend_on_batch_or_regions():
    """the planner's count (host logic, no GPU): the head is a fixed number of launches, one of which reads the map"""
    sd = synth.vgg16_state(0)
    for key in ("pool.whiten", "whiten"):
        sd[key + ".weight"], sd[key + ".bias"] = torch.eye(512), torch.zeros(512)
    expect = {("gem", True, 3, 1e-6, False, True): 8, ("mac", True, 3, 1e-6, False, False): 4, ("rmac", False, 3, 1e-6, False, False): 3,
              ("spoc", False, 0, 1e-6, False, True): 4, ("gemmp", False, 0, 1e-6, False, False): 2}
    for head, launches in expect.items():
        sdh = dict(sd)
        if head[0] == "gemmp":
            sdh["pool.p"] = torch.ones(512) * 3
        if head[1]:
            sdh["pool.rpool.p"] = sdh["pool.p"]
            if head[0] == "mac":
                del sdh["pool.whiten.weight"], sdh["pool.whiten.bias"]
        net = host_graph()
        x = net.input(3)
        f = engine._vgg16_trunk(net, x, sdh)
        kind, regional = head[0], head[1]
        net.pool_head(f, "mac" if kind == "rmac" else kind, p=sdh.get("pool.p") if kind in ("gem", "gemmp") else None, aggregate=2 if regional else int(kind == "rmac"),
                      rwhiten=(sdh["pool.whiten.weight"], sdh["pool.whiten.bias"]) if regional and "pool.whiten.weight" in sdh else None,
                      whiten=(sdh["whiten.weight"], sdh["whiten.bias"]) if head[5] else None)
        counts = {net.head_launches(n, h, w) for n, h, w in ((1, 512, 512), (32, 1024, 1024), (2, 1024, 352), (3, 160, 1152))}
        assert counts == {(launches, 1)}, (head, counts)


def test_plain_gem_embedder_is_planned_as_before():
    """the hub configuration keeps its own op: same ops, same plan, same scratch as before the heads were added (figures of the parent revision)"""
    lib = _hip.load()
    for arch, sd, expect in (("vgg16", synth.vgg16_state(0), PARENT_PLAN["vgg16"]), ("resnet101", synth.resnet101_state(0), PARENT_PLAN["resnet101"])):
        net = host_graph()
        x = net.input(3)
        f = engine._resnet_trunk(net, x, sd) if arch == "resnet101" else engine._vgg16_trunk(net, x, sd)
        net.gem_l2n(f, 3.0)
        got = []
        for n, h, w in ((1, 512, 512), (32, 1024, 1024)):
            b = ctypes.c_size_t()
            _hip.check(lib.gdt_net_workspace_bytes(net.handle, n, h, w, ctypes.byref(b)))
            plan = list(net.plan_summary(n, h, w).values())            # the twelve counters of that revision, in its order; the later ones count nothing here
            assert plan[12:] == [0] * (len(plan) - 12), (arch, plan)
            got.append((lib.gdt_net_num_ops(net.handle), tuple(plan[:12]), b.value))
        assert got == expect, (arch, got)
        assert net.head_launches(1, 512, 512) == (0, 0)


# (ops, plan summary, workspace bytes) at 1 x 512^2 and 32 x 1024^2, computed with the library of the revision before the heads were added
PARENT_PLAN = {"vgg16": [(19, (13, 0, 0, 0, 0, 0, 4, 1, 0, 0, 0, 0), 46137600), (19, (13, 0, 0, 0, 0, 0, 4, 1, 0, 0, 0, 0), 5905580288)],
               "resnet101": [(107, (101, 0, 0, 0, 3, 0, 1, 1, 0, 0, 0, 0), 27263232), (107, (45, 6, 22, 21, 3, 0, 1, 1, 0, 0, 0, 0), 2415919360)]}
