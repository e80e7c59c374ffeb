"""The graph's non-conv ops (csrc/aux_kernels.hip) on the device, each against a float64 evaluation on the tensor it consumed (tapped with output_nchw) under the
derived per-element bounds of tests/aux_bound.py: InstanceNorm on its separate statistics pass, the input pack with a resize, the HED head at sizes that do not
halve exactly, the in-graph GeM + L2N, and the tap with a bias.  Each test prints max |d| / bound, asserts <= 1, and asserts that a second run is bit-identical.
tests/test_aux_bound_cpu.py holds the same bounds against emulated correct and wrong kernels.

Measured figures (MI355X) are in the docstrings of the tests."""
import math

import pytest
import torch

import aux_bound as ab
from gandtr_amd.engine import HipNet
from gandtr_amd.tools import synth

pytestmark = pytest.mark.gpu

PRECISIONS = ["f16", "f16x3"]           # fp16 tensors; the fp32 tensors of the exact-split mode


def _run_twice(net, x, **kw):
    """the outputs of a forward on the CPU, after asserting that a second forward gives the same bits"""
    outs = [o.cpu() for o in net.forward(x, **kw)]
    again = [o.cpu() for o in net.forward(x, **kw)]
    assert len(outs) == len(again) and all(torch.equal(a, b) for a, b in zip(outs, again)), "not bit-identical run to run"
    return outs


# ------------------------------------------------------------------------------------------------ InstanceNorm, separate statistics pass
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", ab.INORM_CASES, ids=ab.case_id)
def test_instance_norm_separate_statistics(cuda_device, case, precision):
    """input(3) -> 1x1 conv with bias (|mean| / std of the channels up to ~2; ~6 in the last case) -> tap -> InstanceNorm in its four forms -> taps.  H W is no
    multiple of 128, so in_stats_kernel / in_finalize_kernel take the statistics from the stored tensor, chunk by chunk; the LeakyReLU form always does.  Bound:
    aux_bound.stat_errors (derived from the chunk length, not the measured STAT_ERR_*) through conv_bound.norm_value, then the store (aux_bound.instance_norm).

    MEASURED on an MI355X, max |d| / bound over the four forms (plain, ReLU, residual, LeakyReLU), cases in the order of aux_bound.INORM_CASES:
    f16    960 px 0.861 0.861 0.951 0.861 | 1025 px 0.932 0.905 0.960 0.904 | 2115 px 0.925 0.925 0.963 0.925 | 15 px 0.989 0.968 0.991 0.978 | 1023 px 0.871 0.871
           0.954 0.871 | 960 px, bias std 1.5: 0.874 0.873 0.924 0.873       (the half ulp of the fp16 store)
    f16x3  960 px 0.005 0.005 0.006 0.005 | 1025 px 0.009 0.009 0.011 0.008 | 2115 px 0.004 0.004 0.007 0.004 | 15 px 0.132 0.129 0.172 0.122 | 1023 px 0.003 0.003
           0.005 0.003 | 960 px, bias std 1.5: 0.006 0.006 0.007 0.006       (the bound allows every summation order; the kernel's is far from the worst)
    The kernels are correct on the chunked path.  Wrong ones under this bound: tests/test_aux_bound_cpu.py (variance without m * m >= 320, unbiased variance
    >= 1.37, one pixel left out >= 23, last chunk left out >= 7000)."""
    (n, c, h, w), bias_std = case
    net = HipNet(cuda_device, precision)
    t = net.input(3)
    a = net.conv(t, synth._normal(11, "wa", (c, 3, 1, 1), 0.7), synth._normal(11, "ba", (c,), bias_std))
    b = net.conv(t, synth._normal(11, "wb", (c, 3, 1, 1), 0.7))
    ta, tb = net.output_nchw(a), net.output_nchw(b)
    slots = {"plain": net.output_nchw(net.instance_norm(a)), "relu": net.output_nchw(net.instance_norm(a, relu=True)),
             "residual": net.output_nchw(net.instance_norm(a, residual=b)), "leaky": net.output_nchw(net.instance_norm(a, leaky=ab.SLOPE))}
    net.finalize()
    assert (h * w) % 128 != 0 and net.plan_summary(n, h, w)["norms_folded"] == 0
    outs = _run_twice(net, synth.synth_input(11, (n, 3, h, w)).to(cuda_device))
    A, B = outs[ta], outs[tb]
    assert tuple(A.shape) == (n, c, h, w)
    if precision == "f16":
        assert torch.equal(A, A.half().float())
    qs = [ab.assert_within(outs[slots[form]], ab.instance_norm(A, form, residual=B, out_f32=precision != "f16"), "InstanceNorm %s %s %s" % (ab.case_id(case), precision, form))
          for form in ab.FORMS]
    print("InstanceNorm %s %s: %s" % (ab.case_id(case), precision, " ".join("%.3f" % q for q in qs)))


# ------------------------------------------------------------------------------------------------ input pack with resize
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", ab.PACK_CASES, ids=ab.case_id)
def test_input_pack_resize_against_float64(cuda_device, case, precision):
    """input(C) -> tap with forward(scale=s): F.interpolate(scale_factor=s, bilinear, align_corners=False) inside pack_input_kernel, with a channel permutation and an
    affine in the last case.  Reference: torch's source coordinate in fp32 exactly as aten takes it (rscale = fp32(1 / s)), everything else in float64.  Bound
    (aux_bound.bilinear, aux_bound.pack_input): one fp32 ulp of the coordinate per axis times the largest tap difference along it (the compiler may contract the
    multiply-subtract; a floor that flips at an integer is covered by continuity), 2 u per axis for the weights, 8 u max |taps| for the arithmetic, the affine's two
    roundings, the fp16 store.  The pre-store error this allows is ~3e-5, against the 4e-3 of test_hip_layers.py::test_input_pack_and_resize.

    MEASURED on an MI355X, max |d| / bound, cases in the order of aux_bound.PACK_CASES:
    f16    0.940 0.937 0.956 0.933 0.980 0.939 0.899 0.922       (the half ulp of the fp16 store)
    f16x3  0.204 0.018 0.288 0.032 0.327 0.242 0.016 0.203       (scale 0.5 lands on lambda = 0.5 exactly; the others are the coordinate's rounding)"""
    shape, s, affine = case
    kw = dict(zip(("perm", "scale", "shift"), affine)) if affine else {}
    net = HipNet(cuda_device, precision)
    o = net.output_nchw(net.input(shape[1], **kw))
    net.finalize()
    x = synth.synth_input(5, shape)
    got = _run_twice(net, x.to(cuda_device), scale=s)[o][:, :shape[1]]
    assert tuple(got.shape[2:]) == HipNet.resized_size(shape[2], shape[3], s)
    ab.assert_within(got, ab.pack_input(x, s, precision != "f16", **kw), "input pack %s %s" % (ab.case_id(case), precision))


# ------------------------------------------------------------------------------------------------ HED head
HED_CHANNELS = (8, 16, 64, 128, 512)    # hed_score_kernel: fewer than 64 channels (one lane group), exactly 64, several passes
HED_INPUTS = [(2, 3, 37, 53),           # maps 37x53, 18x26, 9x13, 4x6, 2x3: ratios like 37/18 and 53/6
              (1, 3, 33, 17),           # 33x17, 16x8, 8x4, 4x2, 2x1
              (2, 3, 16, 24)]           # the dyadic control: exact halvings
HED_FUSION_W, HED_FUSION_B = (0.4, -0.3, 0.25, -0.35, 0.3), 0.1
HED_SCORE_B = (0.3, -0.2, 0.15, -0.1, 0.25)
# 1 / (1 + expf(-v)) against float64 sigmoid of the device's own pre-sigmoid output, in units of u = 2^-24 of the result: MEASURED on an MI355X over the six cases
# below 1.89, 1.96, 1.79, 1.83, 1.81, 1.71 (f16 and f16x3 of each input in turn), largest 1.96; allowed: twice that
SIGMOID_U = 2 * 1.96


def _hed_net(dev, precision):
    """f1 = ReLU 1x1 conv of the input, f(k+1) = ReLU 1x1 conv of maxpool(fk, 2, 2), all five tapped; the head without and with the sigmoid"""
    net = HipNet(dev, precision)
    x, cin, feats, taps = net.input(3), 3, [], []
    for k, c in enumerate(HED_CHANNELS):
        if k:
            x = net.maxpool(x, 2, 2)
        x = net.conv(x, synth._normal(30, "w%d" % k, (c, cin, 1, 1), 1.2 / math.sqrt(cin)), synth._normal(30, "b%d" % k, (c,), 0.3), relu=True)
        feats.append(x)
        taps.append(net.output_nchw(x))
        cin = c
    score_w = [synth._normal(31, "s%d" % k, (c,), 1.0 / math.sqrt(c)) for k, c in enumerate(HED_CHANNELS)]
    pre = net.hed_head(feats, score_w, HED_SCORE_B, HED_FUSION_W, HED_FUSION_B, sigmoid=False)
    sig = net.hed_head(feats, score_w, HED_SCORE_B, HED_FUSION_W, HED_FUSION_B, sigmoid=True)
    net.finalize()
    return net, taps, score_w, pre, sig


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", HED_INPUTS, ids=lambda v: "x".join(str(e) for e in v))
def test_hed_head_at_sizes_that_do_not_halve(cuda_device, shape, precision):
    """hed_score_kernel + hed_fuse_kernel on a mini-net (no VGG) whose floor-pooled pyramid gives bilinear source coordinates that are not dyadic.  Reference: float64
    scores of the five tapped maps, upsampling with the coordinate in fp32 as torch and the kernel both take it (scale = fp32(h) / H) and float64 from there, fusion,
    sigmoid.  Bound (aux_bound.hed_head): score g_(C+1) (sum |x| |w| + |b|); interpolation as in the input pack test, the score error carried by the taps; fusion
    sum |fw_k| e_k + g_6 (sum |fw_k v_k| + |fb|); sigmoid: 1 / 4 of that plus SIGMOID_U u of the result (measured, see above).

    MEASURED on an MI355X, max |d| / bound as (sigmoid=False, sigmoid=True), cases in the order of HED_INPUTS:
    f16    (0.002, 0.003) (0.001, 0.002) (0.002, 0.002)
    f16x3  (0.003, 0.003) (0.001, 0.002) (0.001, 0.002)
    The bound is dominated by g_513 of the 512-channel score, a worst case over all summation orders that a dot product of random signs stays far below; a wrong
    source coordinate moves the output by the maps' tap differences, thousands of times the bound (tests/test_aux_bound_cpu.py: the same interpolation without
    its half-pixel offset).  The non-dyadic sizes behave as the dyadic control."""
    net, taps, score_w, pre, sig = _hed_net(cuda_device, precision)
    n, _, H, W = shape
    outs = _run_twice(net, synth.synth_input(8, shape).to(cuda_device))
    feats = [outs[t] for t in taps]
    sizes, (h, w) = [], (H, W)
    for _ in HED_CHANNELS:
        sizes.append((h, w))
        h, w = h // 2, w // 2
    assert [tuple(f.shape) for f in feats] == [(n, c) + s for c, s in zip(HED_CHANNELS, sizes)]
    r = ab.hed_head(feats, score_w, HED_SCORE_B, HED_FUSION_W, HED_FUSION_B, (H, W))
    label = "HED head %s %s" % ("x".join(str(e) for e in shape), precision)
    got_pre, got_sig = outs[pre].reshape(n, 1, H, W), outs[sig].reshape(n, 1, H, W)
    ab.assert_within(got_pre, r, label + " sigmoid=False")
    own = torch.sigmoid(got_pre.double())
    print("%s: sigmoid against float64 sigmoid of the device's pre-sigmoid output: %.2f u of the result" % (label, float(((got_sig.double() - own).abs() / (ab.U32 * own)).max())))
    ab.assert_within(got_sig, ab.hed_sigmoid(r, SIGMOID_U), label + " sigmoid=True")


# ------------------------------------------------------------------------------------------------ in-graph GeM + L2N
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", ab.GEM_CASES, ids=ab.case_id)
def test_gem_l2n_against_float64(cuda_device, case, precision):
    """input(3) -> 1x1 conv 3 -> D with bias (with a ReLU, or without: negative values that the clamp must lift) -> tap -> gem_l2n(p), on maps of 30 pixels (idle
    pixel rows in gem_kernel), 77 and 1023 (H W % 32 != 0), with the cube path (p = 3) and the powf path.  Reference: (mean clamp(x, eps)^p)^(1/p), then
    / (norm + eps), in float64 on the tapped map, with p and 1 / p the fp32 numbers the kernel holds.

    Bound (derived in aux_bound.gem_l2n), relative to |y|.  Per channel: the term's error tau (2 u for the cube, powf's 16 ulp otherwise), g_HW for the sum in any
    order and u for the division give the mean's relative error d; the outer powf(M', q32) turns it into d / p, adds its own 16 ulp and |ln M| |q32 - 1 / p32| for
    the fp32 rounding of 1 / p: rel_c.  Through the norm: the channels' rel_c move ||v|| by R = ||v (1 + rel)|| / ||v|| - 1, its fp32 evaluation adds g_(D+1) for the
    products and the sum in any order and two roundings (sqrtf, + eps): E.  The final division rounds once: |y' / y - 1| <= (1 + rel_c)(1 + u) / (1 - E) - 1.

    MEASURED on an MI355X, max |d| / bound, cases in the order of aux_bound.GEM_CASES:
    f16    0.017 0.016 0.003 0.012 0.007 0.006 0.002 0.004
    f16x3  0.021 0.016 0.003 0.012 0.007 0.006 0.002 0.004
    (powf is far inside its 16 ulp, and g_HW / g_D are worst cases; without the clamp or without the tail pixels the ratio is >= 230, tests/test_aux_bound_cpu.py)"""
    d, (h, w), p, relu = case
    net = HipNet(cuda_device, precision)
    m = net.conv(net.input(3), synth._normal(7, "w", (d, 3, 1, 1), 0.7), synth._normal(7, "b", (d,), 0.5), relu=relu)
    tm = net.output_nchw(m)
    out = net.gem_l2n(m, p)
    net.finalize()
    outs = _run_twice(net, synth.synth_input(7, (2, 3, h, w)).to(cuda_device))
    M = outs[tm]
    assert tuple(M.shape) == (2, d, h, w) and bool((M < 0).any()) == (not relu)
    ab.assert_within(outs[out].reshape(2, d), ab.gem_l2n(M, p), "GeM + L2N %s %s" % (ab.case_id(case), precision))


# ------------------------------------------------------------------------------------------------ tap with a bias
@pytest.mark.parametrize("precision", PRECISIONS)
def test_tap_with_bias_is_one_fp32_addition(cuda_device, precision):
    """output_nchw(t, bias) = fp32(tap) + bias, one fp32 addition per element: bit-exact against the plain tap plus the bias.  Two tensors, because the builder gives
    every internal conv output C = Creal (cout % 8 == 0): a conv output with C = 16, and the input tensor with C = 8 and Creal = 3, whose padding channels carry
    0 + bias.  13 x 19 pixels: H W is no multiple of anything the kernel strides by."""
    net = HipNet(cuda_device, precision)
    t = net.input(3)
    a = net.conv(t, synth._normal(9, "w", (16, 3, 1, 1), 0.7), synth._normal(9, "b", (16,), 0.5))
    ba, bt = synth._normal(9, "tap16", (16,), 1.0), synth._normal(9, "tap8", (8,), 1.0)
    plain_a, bias_a, plain_t, bias_t = net.output_nchw(a), net.output_nchw(a, ba), net.output_nchw(t), net.output_nchw(t, bt)
    net.finalize()
    outs = _run_twice(net, synth.synth_input(9, (2, 3, 13, 19)).to(cuda_device))
    assert tuple(outs[bias_a].shape) == (2, 16, 13, 19) and tuple(outs[bias_t].shape) == (2, 8, 13, 19)
    assert torch.equal(outs[bias_a], outs[plain_a].float() + ba[None, :, None, None])
    assert torch.equal(outs[bias_t], outs[plain_t].float() + bt[None, :, None, None])
    assert bool((outs[plain_t][:, 3:] == 0).all()) and bool(outs[plain_a].abs().max() > 0)
