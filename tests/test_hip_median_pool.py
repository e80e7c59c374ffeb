"""The geometric-median (Weiszfeld) pooling on the device: gdt_geometric_median on its own against the float64 restatement (tests/median_ref.py), every
net case of tests/golden/median_pool.npz against the reference's descriptors in both precision modes, the multi-scale path against the CPU mirror, and
that a changed iteration count reaches the device net.

The kernel's gate is (h w + d + 8) * 2^-24 * max|m_ref| against median_ref on the same (rounded) input: the first-order bound of the last weighted mean
(two h w-term fp32 sums in any order) plus a weight's d-term sum, root and division.  Measured on an MI355X over all the cases below, the worst case uses
0.045 of it (KERNEL_WORST_SHARE; D = 64 in fp16: 0.045, in fp32: 0.039; D = 512: 0.005; D = 2048: 0.002; the share of every case is printed by the tests) --
the same order as the 0.036 the reference's own fp32 op sequence uses on such maps."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_attention_golden as A                               # noqa: E402  (seeded inputs; imports no reference code)
import make_descriptor_heads_golden as H                        # noqa: E402
import make_median_pool_golden as M                             # noqa: E402
import median_ref                                               # noqa: E402
from gandtr_amd import engine                                   # noqa: E402
from gandtr_amd.components.data import wrapper                  # noqa: E402
from gandtr_amd.components.model.network import cirnet          # noqa: E402
from gandtr_amd.components.model.network._hipbacked import ScaledInput   # noqa: E402
from gandtr_amd.tools import synth                              # noqa: E402

# the descriptor gates of the project (tests/test_hip_golden.py): |d - ref|_inf < 1e-3, cosine > 0.9999
GATE_ABS, GATE_COS = 1e-3, 0.9999
# f16x3 (fp32-class convs): the worst error measured over the eight net cases on an MI355X, asserted at four times the measurement (run-to-run and
# box-to-box slack on an error that is rounding noise) and never beyond a tenth of the f16 gates
X3_MEASURED_ABS = 8.941e-08                                      # att-vgg16-gm3; the other seven cases 2.6e-08 .. 8.6e-08
X3_MEASURED_COS_DEFECT = 6.040e-14                               # 1 - cosine (evaluated in float64), cirnet-vgg16-gm3-w; the others 2.3e-14 .. 3.7e-14
X3_CEIL_ABS, X3_CEIL_COS_DEFECT = GATE_ABS / 10, (1.0 - GATE_COS) / 10
KERNEL_WORST_SHARE = 0.045                                       # D 64 fp16, 1 x 3, 3 iterations; D 512: 0.005, D 2048: 0.002; prior / scale cases: 0.03
EPS24 = 2.0 ** -24
INITS = {"cirnet": cirnet.init_cirnet, "att": cirnet.init_cirnet_attention, "inchan": cirnet.init_cirnet_inchan}

MAPS = ((1, 1), (1, 3), (7, 5), (23, 32), (32, 32))
MAP_SEED = 530                                                   # (a seed at which median_ref moves far enough from one iteration count to the next: asserted below)
SMALL_MAPS = ((1, 3), (7, 5))


def iterations_of(hw):
    return (0, 1, 2, 3, 5) if hw in SMALL_MAPS else (0, 1, 2)


def nhwc(x, device, dtype):
    return x.permute(0, 2, 3, 1).contiguous().to(device, dtype)


def gate(h, w, d, ref):
    return (h * w + d + 8) * EPS24 * float(ref.abs().max())


@functools.lru_cache(maxsize=None)
def kernel_case(h, w, d, dtype):
    """(the map rounded to ``dtype``, as fp32 N x D x H x W; {iterations: float64 reference N x D}) -- computed once and shared, never written to.
    A seeded ReLU map of two images with one zeroed position each (on a 1 x 1 map: in the first image alone, the second keeps its vector) and, on maps of
    more than two positions, the middle position scaled by 50"""
    x = torch.relu(synth.synth_input(MAP_SEED + d + 7 * h + w, (2, d, h, w), name="median.map"))
    flat = x.view(2, d, h * w)
    if h * w > 2:
        flat[:, :, (h * w) // 2] *= 50.0
    flat[0, :, 0] = 0.0
    if h * w > 1:
        flat[1, :, h * w - 1] = 0.0
    x = x.to(dtype).float()
    return x, {it: median_ref.nchw(x, it) for it in iterations_of((h, w))}


# ---------------------------------------------------------------------------------------------------------------- gdt_geometric_median
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("d", [64, 512, 2048])
def test_geometric_median_kernel(cuda_device, d, dtype):
    """every iteration count within the gate of median_ref on the same rounded input; the iteration count matters under that gate (asserted on median_ref: a
    dropped or doubled iteration cannot pass); two runs give the same bits; image 1 of the batch gives the bits it gives alone; ones for scale / prior give
    the bits of none"""
    worst = 0.0
    for h, w in MAPS:
        x, refs = kernel_case(h, w, d, dtype)
        xd = nhwc(x, cuda_device, dtype)
        ones = torch.ones((2, h, w), dtype=torch.float32, device=cuda_device)
        its = iterations_of((h, w))
        if h * w > 1:                                                # what makes the gate tell the iteration counts apart
            assert float((refs[1] - refs[0]).abs().max()) >= 1800 * gate(h, w, d, refs[1]), (h, w)
        if (h, w) in SMALL_MAPS:
            for it in (2, 3):
                assert float((refs[it] - refs[it - 1]).abs().max()) >= 16 * gate(h, w, d, refs[it]), (h, w, it)
        for it in its:
            got = engine.geometric_median(xd, it)
            assert got.shape == (2, d) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
            err, g = float((got.cpu().double() - refs[it]).abs().max()), gate(h, w, d, refs[it])
            worst = max(worst, err / g)
            print("D %d %s %dx%d iterations %d: max|d| %.3e = %.3f of the gate" % (d, dtype, h, w, it, err, err / g))
            assert err <= g, (h, w, it, err, g)
            assert torch.equal(got, engine.geometric_median(xd, it)), ("not reproducible", h, w, it)
            assert torch.equal(got[1:], engine.geometric_median(xd[1:].contiguous(), it)), ("depends on the batch", h, w, it)
            assert torch.equal(got, engine.geometric_median(xd, it, scale=ones, prior=ones)), ("scale / prior of ones", h, w, it)
            if (h, w) == (1, 1):                                     # the input vector: exactly for the mean, else (w y) / w -- two roundings
                v = x.flatten(1)
                if it == 0:
                    assert torch.equal(got.cpu(), v)
                else:
                    assert bool(((got.cpu() - v).abs() <= v.abs() * 2.0 ** -23).all())
    print("D %d %s: worst share of the gate %.3f" % (d, dtype, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_all_positions_equal(cuda_device, dtype):
    """every position AT the median: weights of 1e5, no special case and no NaN"""
    for (h, w), d in (((7, 5), 64), ((32, 32), 512)):
        v = torch.relu(synth.synth_input(530 + d, (2, d, 1, 1), name="median.equal")).to(dtype).float()
        x = v.expand(2, d, h, w).contiguous()
        for it in (0, 1, 3):
            got = engine.geometric_median(nhwc(x, cuda_device, dtype), it).cpu()
            assert bool(torch.isfinite(got).all())
            assert float((got.double() - v.flatten(1).double()).abs().max()) <= gate(h, w, d, v), (h, w, it)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("si", range(len(H.LAYER_SIZES)), ids=["%dx%d" % s for s in H.LAYER_SIZES])
def test_prior_and_scale(cuda_device, si, dtype):
    """the reference's attention maps of the same map (tests/golden/attention.npz), normalised and not, as prior weights and as scale, against median_ref"""
    att = np.load(os.path.join(HERE, "golden", "attention.npz"))
    h, w = H.LAYER_SIZES[si]
    for kind in H.LAYER_KINDS:
        x = H.layer_map(si, kind).to(dtype).float()
        xd = nhwc(x, cuda_device, dtype)
        for nmax in (False, True):
            a = torch.from_numpy(att["att_%d_%s_%d" % (si, kind, nmax)])
            ad = a.to(cuda_device)
            for it in (0, 3):
                for name, kw in (("prior", dict(prior=a)), ("scale", dict(scale=a)), ("both", dict(scale=a, prior=a))):
                    ref = median_ref.nchw(x, it, **kw)
                    got = engine.geometric_median(xd, it, **{k: ad for k in kw})
                    err, g = float((got.cpu().double() - ref).abs().max()), gate(h, w, H.LAYER_D, ref)
                    print("%dx%d %s %s normalize_max %d iterations %d: %.3f of the gate" % (h, w, kind, name, nmax, it, err / g))
                    assert err <= g, (kind, name, nmax, it, err, g)


@pytest.mark.gpu
def test_robustness(cuda_device):
    """one position at 1000 moves the mean, not the median"""
    golden = np.load(os.path.join(HERE, "golden", "median_pool.npz"))
    xd = nhwc(M.outlier_map(), cuda_device, torch.float32)
    mean, med = engine.geometric_median(xd, 0).cpu(), engine.geometric_median(xd, 5).cpu()
    assert float(med.max()) < 0.1 * float(mean.max())
    for it, got in ((0, mean), (5, med)):
        ref = torch.from_numpy(golden["outlier_%d" % it]).double()
        assert float((got.double() - ref).abs().max()) <= 2 * gate(8, 8, 64, ref)       # (the reference's own fp32 evaluation has the same bound)


@pytest.mark.gpu
def test_bad_arguments(cuda_device):
    z = lambda shape, dtype=torch.float32, device=cuda_device: torch.zeros(shape, dtype=dtype, device=device)
    with pytest.raises(ValueError):
        engine.geometric_median(z((1, 4, 4, 32)), 3)                  # channels % 64
    with pytest.raises(ValueError):
        engine.geometric_median(z((1, 4, 4, 96), torch.float16), 3)
    with pytest.raises(ValueError):
        engine.geometric_median(z((1, 4, 4, 64), torch.float64), 3)   # dtype
    with pytest.raises(ValueError):
        engine.geometric_median(z((1, 4, 4, 64), device="cpu"), 3)    # not on the device
    with pytest.raises(ValueError):
        engine.geometric_median(z((1, 4, 4, 64)), 3, scale=z((1, 4, 5)))      # scale of another shape
    with pytest.raises(ValueError):
        engine.geometric_median(z((1, 4, 4, 64)), 3, prior=z((1, 4, 4), torch.float16))
    with pytest.raises(ValueError):
        engine.geometric_median(z((1, 4, 4, 64)), -1)
    with pytest.raises(ValueError):
        engine.geometric_median(z((1, 4, 4, 64)), 65)


# ---------------------------------------------------------------------------------------------------------------- nets
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "median_pool.npz"))


def errors(got, ref):
    got, ref = got.detach().cpu().double(), torch.as_tensor(np.asarray(ref)).double()
    return float((got - ref).abs().max()), float(torch.nn.functional.cosine_similarity(got, ref, dim=0).min())


@pytest.mark.gpu
@pytest.mark.parametrize("case", M.NET_CASES, ids=M.case_name)
def test_nets_f16_against_the_reference(cuda_device, golden, case):
    name = M.case_name(case)
    net = M.build_net(INITS, case, int(golden["net_%s_seed" % name]))
    with torch.no_grad():
        out = net.to(cuda_device)(M.case_input(case).to(cuda_device))
    err, cos = errors(out, golden["net_%s_out" % name])
    print("%s f16: max|d| %.3e  min cosine %.7f" % (name, err, cos))
    assert out.shape == (net.meta["outputdim"], 2)
    assert err < GATE_ABS and cos > GATE_COS, (name, err, cos)
    hip = net._hip_embedder()
    assert hip.head_launches(2, 160, 224)[1] == case[2] + 1


@pytest.mark.gpu
def test_nets_f16x3_against_the_reference(cuda_device, golden):
    worst_err, worst_cos = 0.0, 1.0
    for case in M.NET_CASES:
        name = M.case_name(case)
        net = M.build_net(INITS, case, int(golden["net_%s_seed" % name]))
        net.hip_precision = "f16x3"
        with torch.no_grad():
            out = net.to(cuda_device)(M.case_input(case).to(cuda_device))
        err, cos = errors(out, golden["net_%s_out" % name])
        print("%s f16x3: max|d| %.3e  1 - min cosine %.3e" % (name, err, 1.0 - cos))
        worst_err, worst_cos = max(worst_err, err), min(worst_cos, cos)
    print("f16x3 worst: max|d| %.3e  1 - min cosine %.3e" % (worst_err, 1.0 - worst_cos))
    assert X3_MEASURED_ABS is not None and X3_MEASURED_COS_DEFECT is not None, "the MI355X measurement has not been written into this file"
    assert worst_err <= min(4 * X3_MEASURED_ABS, X3_CEIL_ABS) and 1.0 - worst_cos <= min(4 * X3_MEASURED_COS_DEFECT, X3_CEIL_COS_DEFECT), \
        (worst_err, 1.0 - worst_cos)


@pytest.mark.gpu
def test_multiscale_against_the_cpu_mirror(cuda_device):
    """the pyramid of cirmultiscale through forward_many (meta["pooling"] is the dict: msp = 1)"""
    case = ("cirnet", "vgg16", 3, False, True, None)
    net, x = M.build_net(INITS, case, 1000), M.case_input(case)
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
        print("%s level: max|d| %.3e  min cosine %.7f" % (M.case_name(case), err, cos))
        assert err < GATE_ABS and cos > GATE_COS, (err, cos)


@pytest.mark.gpu
def test_a_changed_iteration_count_reaches_the_device_net(cuda_device, golden):
    net, x = M.build_net(INITS, ("cirnet", "vgg16", 0, False, False, None), 1000), A.att_input()
    net, xd = net.to(cuda_device), x.to(cuda_device)
    with torch.no_grad():
        a = net(xd)
        first = net._hip_embedder()
        net.pool.iterations = 3
        b = net(xd)
        second = net._hip_embedder()
    assert first is not second and first.head_launches(2, 160, 224) == (3, 1) and second.head_launches(2, 160, 224) == (9, 4)
    for out, name in ((a, "cirnet-vgg16-gm0"), (b, "cirnet-vgg16-gm3")):
        err, cos = errors(out, golden["net_%s_out" % name])
        assert err < GATE_ABS and cos > GATE_COS, (name, err, cos)
    assert float((a - b).abs().max()) > 2 * GATE_ABS                 # another descriptor: further apart than two results inside the gate of ONE reference can be
