"""The blur-resample graph op (gdt_net_blur_resample, csrc/blur_resample.hip) on the device through HipNet, in "f16" (fp16 tensors) and "f16x3" (fp32 tensors),
against the float64 evaluations of blur_ref.py under the derived per-element bounds of blur_bound.py.  The net is input(3) -> 1 x 1 conv with a bias (channel
means up to about 2 standard deviations) -> tap -> [InstanceNorm (+ ReLU), folded into the op] -> op -> tap; the reference is evaluated on the tapped RAW tensor.
Each test prints max |d| / bound, asserts <= 1, and asserts that a second run is bit-identical.  tests/test_blur_bound_cpu.py holds the same bounds against
emulated correct and wrong kernels.

Measured figures (MI355X) are in the docstrings of the tests."""
import pytest
import torch

import blur_bound as bb
import blur_ref as br
from gandtr_amd.engine import HipNet

pytestmark = pytest.mark.gpu

PRECISIONS = ["f16", "f16x3"]
CASES = br.cases()


def _run_twice(net, x):
    outs = [o.cpu() for o in net.forward(x)]
    again = [o.cpu() for o in net.forward(x)]
    assert len(outs) == len(again) and all(torch.equal(a, b) for a, b in zip(outs, again)), "not bit-identical run to run"
    return outs


def _net(dev, precision, shape, up, norms):
    """one producer, one op per entry of ``norms`` (None: plain form; "plain" / "relu": behind an InstanceNorm that only the op consumes)"""
    net = HipNet(dev, precision)
    w, b = br.producer_weights(shape[1])
    raw = net.conv(net.input(3), w, b)
    slots = {"raw": net.output_nchw(raw)}
    for norm in norms:
        t = raw if norm is None else net.instance_norm(raw, relu=norm == "relu")
        slots[norm] = net.output_nchw(net.blur_resample(t, up=up))
    net.finalize()
    return net, slots


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=br.case_id)
def test_plain_form_against_float64(cuda_device, case, precision):
    """the op on the stored tensor.  Bound: g_8 sum w |t| (down: exact products, eight additions) / g_5 sum w |t| (up), + the fp16 store in "f16".

    MEASURED on an MI355X, max |d| / bound, cases in the order of blur_ref.cases() (down 2x2 .. 37x53, up 2x2 .. 37x53, 1x4, 3x1):
    f16    0.924 0.744 0.978 0.992 0.999 0.998 | 0.995 0.999 0.987 0.999 0.999 0.999 0.949 0.882       (the half ulp of the fp16 store)
    f16x3  0.139 0.176 0.241 0.294 0.315 0.314 | 0.212 0.235 0.338 0.373 0.365 0.388 0.154 0.189       (the bound allows every order; the kernel's is separable)"""
    shape, up = case
    net, slots = _net(cuda_device, precision, shape, up, [None])
    n, c, h, w = shape
    assert net.blur_summary(n, h, w) == {"launches": 1, "folded": 0}
    outs = _run_twice(net, br.producer_input(shape).to(cuda_device))
    raw = outs[slots["raw"]]
    want = (n, c, 2 * h, 2 * w) if up else (n, c, (h + 1) // 2, (w + 1) // 2)
    assert tuple(raw.shape) == shape and tuple(outs[slots[None]].shape) == want
    bb.assert_within(outs[slots[None]], bb.blur(raw, up, None, out_f32=precision != "f16"), "blur %s %s unfolded" % (br.case_id(case), precision))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=br.case_id)
def test_folded_forms_against_float64_of_the_raw_tensor(cuda_device, case, precision):
    """conv -> InstanceNorm (plain; + ReLU) -> op: the planner folds both norms into their ops (blur_summary), the normalised tensors are never written, and the
    result is held against float64 InstanceNorm + op of the tapped raw tensor.  Bound: the taps' dz (statistics, the two operations of (x - mean) rstd) carried by the
    convex combination, the arithmetic on the grown magnitudes, the store.  At 16 x 16 the 1 x 1 conv delivers the statistics from its epilogue
    (blur_ref.fused_statistics): with fp16 tensors they are the statistics of the results BEFORE the store, bounded by blur_bound.statistics_errors.

    MEASURED on an MI355X, max |d| / bound, cases in the order of blur_ref.cases() (down | up):
    f16    norm         0.032 0.783 0.860 0.303 0.931 0.803 | 0.967 0.923 0.924 0.380 0.983 0.878 0.903 0.927
           norm + ReLU  0.560 0.982 0.891 0.298 0.957 0.805 | 0.903 0.923 0.945 0.355 0.984 0.871 0.903 0.831
                        (the fp16 store; 16 x 16, the fourth of either group, is held to the looser epilogue-statistics bound: 0.30 - 0.38 of it)
    f16x3  norm         0.056 0.076 0.050 0.007 0.042 0.003 | 0.128 0.156 0.063 0.012 0.058 0.004 0.122 0.152
           norm + ReLU  0.070 0.076 0.049 0.008 0.036 0.003 | 0.109 0.156 0.063 0.011 0.069 0.004 0.091 0.152
                        (the statistics' worst case over all summation orders dominates the bound; the kernels' sums are far from it)"""
    shape, up = case
    net, slots = _net(cuda_device, precision, shape, up, ["plain", "relu"])
    n, c, h, w = shape
    assert net.blur_summary(n, h, w) == {"launches": 2, "folded": 2} and net.plan_summary(n, h, w)["norms_folded"] == 2
    outs = _run_twice(net, br.producer_input(shape).to(cuda_device))
    raw = outs[slots["raw"]]
    qs = [bb.assert_within(outs[slots[norm]], bb.blur(raw, up, norm, out_f32=precision != "f16", fused=br.fused_statistics(shape)),
                           "blur %s %s norm-%s" % (br.case_id(case), precision, norm)) for norm in ("plain", "relu")]
    print("blur folded %s %s: %s" % (br.case_id(case), precision, " ".join("%.3f" % q for q in qs)))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_down_op_refuses_a_one_pixel_axis_and_the_process_lives_on(cuda_device, precision):
    """H = 1: the forward returns the planner's error before anything is launched; the same net then serves a valid geometry (a refusal, not a fault)"""
    shape = (2, 8, 5, 7)
    net, slots = _net(cuda_device, precision, shape, False, [None, "relu"])
    for h, w in [(1, 7), (5, 1)]:
        with pytest.raises(ValueError, match="at least 2 x 2"):
            net.forward(br.producer_input((2, 8, h, w)).to(cuda_device))
    outs = _run_twice(net, br.producer_input(shape).to(cuda_device))
    bb.assert_within(outs[slots[None]], bb.blur(outs[slots["raw"]], False, None, out_f32=precision != "f16"), "blur down after a refusal, %s" % precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_up_op_equals_the_bilinear_resize(cuda_device, precision):
    """Upsample is F.interpolate(scale_factor=2, bilinear): the op's output against net.resize to the op's own size, each within its bound of the same float64 map

    MEASURED on an MI355X: f16 -- up op 0.999 of its bound, resize 0.998, the two outputs bit-identical; f16x3 -- 0.388 and 0.206, max |up - resize| 7.2e-7 =
    0.21 of the two bounds' sum (the op rounds each axis once, the resize kernel every product and sum)"""
    shape = (2, 32, 37, 53)
    net = HipNet(cuda_device, precision)
    w, b = br.producer_weights(shape[1])
    raw = net.conv(net.input(3), w, b)
    up = net.blur_resample(raw, up=True)
    s_raw, s_up, s_rs = net.output_nchw(raw), net.output_nchw(up), net.output_nchw(net.resize(raw, up))
    net.finalize()
    outs = _run_twice(net, br.producer_input(shape).to(cuda_device))
    f32 = precision != "f16"
    r_up, r_rs = bb.blur(outs[s_raw], True, None, out_f32=f32), bb.resize_x2(outs[s_raw], out_f32=f32)
    assert torch.equal(r_up.ref, r_rs.ref)
    bb.assert_within(outs[s_up], r_up, "up op %s" % precision)
    bb.assert_within(outs[s_rs], r_rs, "resize x 2 %s" % precision)
    d = (outs[s_up].double() - outs[s_rs].double()).abs()
    q = float((d / (r_up.bound + r_rs.bound)).max())
    print("up op against resize %s: max |d| = %.3e, max |d| / (bound + bound) = %.3f" % (precision, float(d.max()), q))
    assert q <= 1.0
