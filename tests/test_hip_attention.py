"""The attention and edge-map embedders on the device: the pixel attention kernel and the weighted region pooling on their own (through the C ABI), the
EdgeFilter of the input pack, every net case of tests/golden/attention.npz against the reference's descriptors in both precision modes, the
multi-scale path against the CPU mirror, and that a changed attention setting or filter parameter reaches the device net.

The input pack's filter is gated at 4 * 2^-24 relative + w * 2^-24 absolute of a float64 evaluation of the same formula: measured on an MI355X over
the fixture's inputs, the worst element uses 0.38 of that allowance (parameter set 1; set 0: 0.34) -- the device's powf / expf need no wider gate."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_attention_golden as A                               # noqa: E402  (seeded inputs, case lists; imports no reference code)
import make_descriptor_heads_golden as H                        # noqa: E402
from gandtr_amd import engine                                   # noqa: E402
from gandtr_amd.components.data import wrapper                  # noqa: E402
from gandtr_amd.components.model.network import cirnet          # noqa: E402
from gandtr_amd.components.model.network._hipbacked import ScaledInput   # noqa: E402
from gandtr_amd.tools import synth                              # noqa: E402

# the descriptor gates of the project (tests/test_hip_golden.py): |d - ref|_inf < 1e-3, cosine > 0.9999
GATE_ABS, GATE_COS = 1e-3, 0.9999
# f16x3 (fp32-class convs): the worst error measured over the eleven net cases on an MI355X, asserted at four times the measurement (run-to-run and
# box-to-box slack on an error that is rounding noise) and never beyond a tenth of the f16 gates
X3_MEASURED_ABS = 2.161e-07                                      # att-vgg16-mac-max; the other ten cases 3.0e-08 .. 8.6e-08
X3_MEASURED_COS_DEFECT = 4.144e-13                               # 1 - cosine (evaluated in float64), the same case
X3_CEIL_ABS, X3_CEIL_COS_DEFECT = GATE_ABS / 10, (1.0 - GATE_COS) / 10
EPS24 = 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "attention.npz"))


def nhwc(x, device, dtype):
    return x.permute(0, 2, 3, 1).contiguous().to(device, dtype)


# ---------------------------------------------------------------------------------------------------------------- gdt_pixel_attention
ATT_MAPS = ((1, 3), (7, 5), (23, 32), (32, 32))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("d", [64, 512, 2048])
def test_pixel_attention_kernel(cuda_device, d, dtype):
    """every weight within (D + 4) * 2^-24 relative of a float64 evaluation of the same (rounded) input -- the first-order bound for D squares summed in
    fp32 in any order, plus the square root and the division; the image's maximum has weight exactly 1; two runs give the same bits"""
    for h, w in ATT_MAPS:
        x = torch.relu(synth.synth_input(400 + d + h, (2, d, h, w), name="att.map"))
        x[1] *= 3.0                                                      # images of different maxima
        x[0, :, 0, 0] = 0.0                                              # a position where only the 1e-10 is left
        x = x.to(dtype).float()
        xd = nhwc(x, cuda_device, dtype)
        m = (x.double().pow(2).sum(1) + 1e-10).sqrt()                   # N x H x W
        for nmax in (False, True):
            ref = m / m.flatten(1).max(dim=1).values.view(-1, 1, 1) if nmax else m
            got = engine.pixel_attention(xd, nmax)
            rel = float(((got.cpu().double() - ref).abs() / ref).max())
            print("D %d %s %dx%d normalize_max %d: max rel %.3e (%.2f of the bound)" % (d, dtype, h, w, nmax, rel, rel / ((d + 4) * EPS24)))
            assert got.shape == (2, h, w) and got.dtype == torch.float32
            assert rel <= (d + 4) * EPS24, (h, w, nmax, rel)
            assert torch.equal(got, engine.pixel_attention(xd, nmax)), ("not reproducible", h, w, nmax)
            if nmax:
                flat = got.flatten(1)
                assert (flat.max(dim=1).values == 1.0).all() and torch.equal(flat.argmax(dim=1).cpu(), ref.flatten(1).argmax(dim=1))
            else:
                assert float(got[0, 0, 0]) == pytest.approx(1e-5, rel=4 * EPS24)


@pytest.mark.gpu
def test_pixel_attention_bad_arguments(cuda_device):
    with pytest.raises(ValueError):
        engine.pixel_attention(torch.zeros((1, 4, 4, 32), dtype=torch.float32, device=cuda_device))        # channels % 64
    with pytest.raises(ValueError):
        engine.pixel_attention(torch.zeros((1, 4, 4, 96), dtype=torch.float16, device=cuda_device))
    with pytest.raises(ValueError):
        engine.pixel_attention(torch.zeros((1, 4, 4, 64), dtype=torch.float64, device=cuda_device))
    with pytest.raises(ValueError):
        engine.pixel_attention(torch.zeros((1, 4, 4, 64), dtype=torch.float32))                              # not on the device
    with pytest.raises(ValueError):
        engine.pool_regions_weighted(torch.zeros((1, 4, 4, 64), dtype=torch.float32, device=cuda_device),
                                     torch.ones((1, 4, 5), dtype=torch.float32, device=cuda_device), "mac")    # weights of another shape
    with pytest.raises(ValueError):
        engine.pool_regions_weighted(torch.zeros((1, 4, 4, 64), dtype=torch.float32, device=cuda_device),
                                     torch.ones((1, 4, 4), dtype=torch.float32, device=cuda_device), "gemmp")  # per-channel GeM without its exponents


# ---------------------------------------------------------------------------------------------------------------- gdt_pool_regions_weighted
def host_regions(x, pool, levels):
    if levels == 0:
        return pool(x).flatten(1).unsqueeze(1)
    return cirnet.roipool(x, pool, levels).flatten(2)


def unweighted(xd, kind, p, pch, levels):
    """gdt_pool_regions, as tests/test_hip_descriptor_heads.py calls it"""
    import ctypes
    from gandtr_amd import _hip
    lib = _hip.load()
    n, h, w, d = xd.shape
    cnt = ctypes.c_int()
    _hip.check(lib.gdt_rpool_regions(h, w, levels, None, 0, ctypes.byref(cnt)))
    out = torch.full((n, cnt.value, d), float("nan"), dtype=torch.float32, device=xd.device)
    with torch.cuda.device(xd.device):
        _hip.check(lib.gdt_pool_regions(xd.data_ptr(), int(xd.dtype == torch.float32), n, h, w, d, engine.HipNet.POOL_KINDS[kind], float(p),
                                        None if pch is None else pch.data_ptr(), 1e-6, levels, out.data_ptr(),
                                        torch.cuda.current_stream(xd.device).cuda_stream))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("si", range(len(H.LAYER_SIZES)), ids=["%dx%d" % s for s in H.LAYER_SIZES])
def test_weighted_region_pooling_kernel(cuda_device, golden, si, dtype):
    """weights: the reference's attention maps of the same map, normalised and not.  max: bit-exact against (x * a) pooled on the host (one fp32
    multiply on both sides); mean / GeM kinds: within 1e-5 * max(1, max a) of float64 (the unweighted kernel's 1e-5, scaled by how much the weights
    scale the map); two runs give the same bits; weights of one give the unweighted kernel's bits"""
    p_mp = H.layer_params()[0]
    p_dev = p_mp.to(cuda_device)
    for kind in H.LAYER_KINDS:
        x = H.layer_map(si, kind).to(dtype).float()
        xd = nhwc(x, cuda_device, dtype)
        for nmax in (False, True):
            a = torch.from_numpy(golden["att_%d_%s_%d" % (si, kind, nmax)])          # N x H x W
            ad = a.to(cuda_device)
            gate = 1e-5 * max(1.0, float(a.max()))
            xa, xa64 = x * a.unsqueeze(1), x.double() * a.double().unsqueeze(1)
            for levels in (0, 3):
                got = engine.pool_regions_weighted(xd, ad, "mac", levels=levels)
                assert torch.equal(got.cpu(), host_regions(xa, cirnet.mac, levels)), ("mac", kind, nmax, levels)
                cases = {"spoc": (cirnet.spoc, 1.0, None), "gem": (lambda t: cirnet.gem(t, 2.37), 2.37, None),
                         "gemmp": (lambda t: cirnet.gem(t, p_mp.double().view(1, -1, 1, 1)), 1.0, p_dev)}
                for name, (pool, p, pch) in cases.items():
                    got = engine.pool_regions_weighted(xd, ad, name, p=p, p_channels=pch, levels=levels)
                    ref = host_regions(xa64, pool, levels)
                    err = float((got.cpu().double() - ref).abs().max())
                    print("%s %s %s normalize_max %d levels %d: max|d| %.3e (gate %.3e)" % (H.LAYER_SIZES[si], kind, name, nmax, levels, err, gate))
                    assert got.shape == ref.shape and err <= gate, (name, kind, nmax, levels, err)
                    assert torch.equal(got, engine.pool_regions_weighted(xd, ad, name, p=p, p_channels=pch, levels=levels)), ("not reproducible", name)
        ones = torch.ones(x.shape[0], x.shape[2], x.shape[3], dtype=torch.float32, device=cuda_device)
        for levels in (0, 3):
            for name, p, pch in (("mac", 1.0, None), ("spoc", 1.0, None), ("gem", 3.0, None), ("gem", 2.37, None), ("gemmp", 1.0, p_dev)):
                assert torch.equal(engine.pool_regions_weighted(xd, ones, name, p=p, p_channels=pch, levels=levels), unweighted(xd, name, p, pch, levels)), \
                    ("weights of one", name, p, kind, levels)


# ---------------------------------------------------------------------------------------------------------------- the filter in the input pack
def filter_f64(x, params, tau):
    x = x.double()
    p32 = float(np.float32(params["p"]))
    gate = torch.exp((-params["beta"] * (x - tau)).clamp(max=50.0)) + 1
    return params["w"] * x.clamp(min=params["eps"]).pow(p32) / gate


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(A.FILTER_SETS)))
def test_input_pack_filter(cuda_device, golden, k):
    """the fp32 output form against a float64 evaluation of the formula on the same input (4 * 2^-24 relative + w * 2^-24 absolute), and against the
    reference's own fp32 output with that output's own distance from float64 added; the fp16 form is the fp32 form rounded"""
    params = A.filter_params(k)
    tau = float(golden["filter_%d_tau" % k][0])                           # clamped, as the reference left it
    x = A.filter_input()
    ref64 = filter_f64(x, params, tau)
    gate = 4 * EPS24 * ref64.abs() + params["w"] * EPS24
    filt = ("edgefilter", params["w"], params["p"], params["beta"], params["tau"], params["eps"])       # the unclamped tau: the library clamps
    got = engine.pack_input_filter(x.to(cuda_device), filt, out_f32=True)
    assert got.shape == (2, 24, 40, 8) and not got[..., 1:].any()
    y = got[..., 0].cpu().unsqueeze(1)
    used = float(((y.double() - ref64).abs() / gate).max())
    print("filter set %d: worst element uses %.3f of the float64 gate" % (k, used))
    assert used <= 1.0
    ref32 = torch.from_numpy(golden["filter_%d_out" % k])
    assert bool(((y.double() - ref32.double()).abs() <= gate + (ref32.double() - ref64).abs()).all())
    half = engine.pack_input_filter(x.to(cuda_device), filt, out_f32=False)
    assert torch.equal(half[..., 0].cpu().unsqueeze(1), y.half())
    three = engine.pack_input_filter(x.expand(-1, 3, -1, -1).contiguous().to(cuda_device), filt)
    assert torch.equal(three[..., 1], got[..., 0]) and torch.equal(three[..., 2], got[..., 0]) and not three[..., 3:].any()


# ---------------------------------------------------------------------------------------------------------------- nets
def net_cases():
    return [("att", c) for c in A.ATT_CASES] + [("inchan", c) for c in A.INCHAN_CASES]


def case_id(kc):
    return A.att_name(kc[1]) if kc[0] == "att" else A.inchan_name(kc[1])


def build(kc, seed):
    kind, case = kc
    if kind == "att":
        return A.build_att_net(cirnet.init_cirnet_attention, case, seed), A.att_input()
    return A.build_inchan_net(cirnet.init_cirnet_inchan, case, seed), A.net_input(case[1])


def errors(got, ref):
    got, ref = got.detach().cpu().double(), torch.as_tensor(np.asarray(ref)).double()
    return float((got - ref).abs().max()), float(torch.nn.functional.cosine_similarity(got, ref, dim=0).min())


@pytest.mark.gpu
@pytest.mark.parametrize("kc", net_cases(), ids=case_id)
def test_nets_f16_against_the_reference(cuda_device, golden, kc):
    name = case_id(kc)
    net, x = build(kc, int(golden["net_%s_seed" % name]))
    with torch.no_grad():
        out = net.to(cuda_device)(x.to(cuda_device))
    err, cos = errors(out, golden["net_%s_out" % name])
    print("%s f16: max|d| %.3e  min cosine %.7f" % (name, err, cos))
    assert out.shape == (net.meta["outputdim"], 2)
    assert err < GATE_ABS and cos > GATE_COS, (name, err, cos)


@pytest.mark.gpu
def test_nets_f16x3_against_the_reference(cuda_device, golden):
    worst_err, worst_cos = 0.0, 1.0
    for kc in net_cases():
        name = case_id(kc)
        net, x = build(kc, int(golden["net_%s_seed" % name]))
        net.hip_precision = "f16x3"
        with torch.no_grad():
            out = net.to(cuda_device)(x.to(cuda_device))
        err, cos = errors(out, golden["net_%s_out" % name])
        print("%s f16x3: max|d| %.3e  1 - min cosine %.3e" % (name, err, 1.0 - cos))
        worst_err, worst_cos = max(worst_err, err), min(worst_cos, cos)
    print("f16x3 worst: max|d| %.3e  1 - min cosine %.3e" % (worst_err, 1.0 - worst_cos))
    assert worst_err <= min(4 * X3_MEASURED_ABS, X3_CEIL_ABS) and 1.0 - worst_cos <= min(4 * X3_MEASURED_COS_DEFECT, X3_CEIL_COS_DEFECT), \
        (worst_err, 1.0 - worst_cos)


@pytest.mark.gpu
@pytest.mark.parametrize("kc", [("att", ("vgg16", "gem", True, True)), ("inchan", ("vgg16", 1, True))], ids=case_id)
def test_multiscale_against_the_cpu_mirror(cuda_device, kc):
    """the pyramid of cirmultiscale through forward_many: on the device the resize and, behind it, the filter are the input pack's"""
    net, x = build(kc, 1000)
    ms_cpu = wrapper.CirMultiscaleAggregation("ms", torch.device("cpu"))
    with torch.no_grad():
        refs = [net(l) for l in ms_cpu.preprocess(x, net)[0]]
    net = net.to(cuda_device)
    levels, _ = wrapper.CirMultiscaleAggregation("ms", cuda_device).preprocess(x.to(cuda_device), net)
    assert all(isinstance(l, ScaledInput) for l in levels) and len(levels) == 3
    with torch.no_grad():
        many = net.forward_many(levels)
        single = [net(l) for l in levels]
    torch.cuda.synchronize(cuda_device)
    for a, b, ref in zip(many, single, refs):
        assert torch.equal(a, b)
        err, cos = errors(a, ref)
        print("%s level: max|d| %.3e  min cosine %.7f" % (case_id(kc), err, cos))
        assert err < GATE_ABS and cos > GATE_COS, (err, cos)


@pytest.mark.gpu
def test_changed_settings_reach_the_device_net(cuda_device, golden):
    """normalize_max is part of the device net's key; the filter's tau is a parameter, whose new value a load_state_dict brings to the device"""
    net, x = build(("att", ("vgg16", "gem", False, False)), 1000)
    net, xd = net.to(cuda_device), x.to(cuda_device)
    with torch.no_grad():
        a = net(xd)
        first = net._hip_embedder()
        net.attention.normalize_max = True
        b = net(xd)
        second = net._hip_embedder()
    assert first is not second and first.attention_launches(2, 160, 224) == (1, 2) and second.attention_launches(2, 160, 224) == (2, 2)
    for out, name in ((a, "att-vgg16-gem"), (b, "att-vgg16-gem-max")):
        err, cos = errors(out, golden["net_%s_out" % name])
        assert err < GATE_ABS and cos > GATE_COS, (name, err, cos)
    rmac, _ = build(("att", ("vgg16", "rmac", False, True)), 1000)
    rmac.attention.normalize_max = False
    with torch.no_grad():
        ref = rmac(x)
        out = rmac.to(cuda_device)(xd)
    err, cos = errors(out, ref)
    assert err < GATE_ABS and cos > GATE_COS, (err, cos)

    net, x = build(("inchan", ("vgg16", 1, True)), 1000)
    moved = {k: v.clone() for k, v in net.state_dict().items()}
    moved["preprocessing.tau"].fill_(0.5)
    dev = A.build_inchan_net(cirnet.init_cirnet_inchan, ("vgg16", 1, True), 1000).to(cuda_device)
    with torch.no_grad():
        before = dev(x.to(cuda_device))
        dev.load_state_dict(moved)
        after = dev(x.to(cuda_device))
        net.load_state_dict(moved)
        ref = net(x)
    assert float((before - after).abs().max()) > 10 * GATE_ABS                  # the step moved from 0.1 to 0.5: another descriptor
    err, cos = errors(after, ref)
    assert err < GATE_ABS and cos > GATE_COS, (err, cos)
