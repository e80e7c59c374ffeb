"""Every f16 conv family alone behind a 1 x 1 lift: the variant code the dispatcher reports for the layer is asserted, every output is held to the derived bound of
tests/conv_bound.py (float64 reference on the fp16 tensors the layer consumed), and an unprofiled forward equals the profiled one bit for bit.  Shapes are the smallest
that default knobs send to the kernel named, one ragged and one whole-tile case per family.  The ratios max |d| / bound are printed per case (DESIGN.md lists them)."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_bound as cb
from gandtr_amd.tools import synth

pytestmark = pytest.mark.gpu


def _bn(seed, cout):
    return (synth._uniform(seed, "g", (cout,), 0.5, 1.5), synth._normal(seed, "be", (cout,), 0.2), synth._normal(seed, "m", (cout,), 0.2), synth._uniform(seed, "v", (cout,), 0.5, 1.5))


def _conv_variants(net):
    return [v for k, v, ms, fl in net.profile() if k == 1]


def _run(dev, cin, cout, shape, variant, k=3, stride=1, pad=None, reflect=False, transposed=False, dilation=1, relu=False, bn=False, pool=False, residual=False,
         norm=None, stats=False, seed=0, label=""):
    """one layer behind a 1 x 1 lift.  ``norm``: None, "relu" (InstanceNorm + ReLU consumed by the layer alone: folded), "wb" (the same, read by a second consumer: folded
    with write-back), "res" (InstanceNorm + residual: folded, written back unless the layer is the fused transposed conv).  ``stats``: an InstanceNorm follows, its
    statistics come from the layer's epilogue."""
    from gandtr_amd.engine import HipNet
    n, h, w = shape
    pad = (dilation * (k // 2)) if pad is None else pad
    g = lambda name, shp, std: synth._normal(seed, name, shp, std)
    net = HipNet(dev)
    t = net.input(3)
    a = net.conv(t, g("w0", (cin, 3, 1, 1), 0.7))
    tap_in = net.output_nchw(a)
    n_lifts = 1
    tap_r = tap_res = res_t = None
    u = a
    if norm == "res":
        r0 = net.conv(t, g("w1", (cin, 3, 1, 1), 0.7))
        tap_r = net.output_nchw(r0)
        n_lifts += 1
        u = net.instance_norm(a, relu=False, residual=r0)
    elif norm:
        u = net.instance_norm(a, relu=True)
    if residual:
        res_t = net.conv(t, g("w2", (cout, 3, 1, 1), 0.7), stride=stride)
        tap_res = net.output_nchw(res_t)
        n_lifts += 1
    wt = g("w", (cin, cout, k, k) if transposed else (cout, cin, k, k), math.sqrt(2.0 / (cin * k * k / (4 if transposed else 1))))
    bias = g("b", (cout,), 0.2)
    bnp = _bn(seed, cout) if bn else None
    o = net.conv(u, wt, bias, bn=bnp, stride=stride, pad=pad, reflect=reflect, transposed=transposed, relu=relu, residual=res_t if residual else -1, dilation=dilation)
    tap_wb = net.output_nchw(u) if norm == "wb" or (norm == "res" and not transposed) else None       # (after the conv in program order: the conv writes the tensor back)
    tap = net.output_nchw(net.maxpool(o, 2, 2) if pool else o)
    tap_n = net.output_nchw(net.instance_norm(o, relu=True)) if stats else None
    net.finalize()
    x = synth.synth_input(seed + 1, (n, 3, h, w)).to(dev)
    net.set_profiling(True)
    outs = [t_.cpu() for t_ in net.forward(x)]
    torch.cuda.synchronize()
    variants = _conv_variants(net)
    net.set_profiling(False)
    again = net.forward(x)
    xin = outs[tap_in]
    assert torch.equal(cb.f16(xin), xin)
    in_delta = None
    if norm:
        ain, in_delta = cb.norm_input(xin, relu=norm != "res", residual=outs[tap_r] if norm == "res" else None)
    else:
        ain = xin
    wp, shift = cb.fold(wt, bias, bnp, transposed)
    print("%s: variants %s" % (label, variants))
    q = cb.assert_layer(outs[tap], ain, wp, shift, label, in_delta=in_delta, residual=outs[tap_res] if residual else None, stride=stride, pad=pad, reflect=reflect,
                        dilation=dilation, transposed=transposed, act="relu" if relu else None, pool=pool)
    if tap_wb is not None:                  # the tensor the conv wrote back: what it staged
        dwb = (outs[tap_wb].double() - ain).abs()
        print("%s: write-back max |d| / bound = %.3f" % (label, float((dwb / in_delta).max())))
        assert bool((dwb <= in_delta).all()), label
    if stats:                               # the InstanceNorm behind the layer, its statistics taken in the epilogue, against the norm of the layer's own output
        want, dn = cb.norm_input(outs[tap], relu=True)
        dq = float(((outs[tap_n].double() - want).abs() / dn).max())
        print("%s: following InstanceNorm max |d| / bound = %.3f" % (label, dq))
        assert dq <= 1.0, label
    assert variants[n_lifts] == variant, (label, variants)
    assert all(torch.equal(p, q_.cpu()) for p, q_ in zip(outs, again)), label
    return q


def _id(c):
    return c[0]


# ---- conv3x3_halo_rb.hip, 256-column forms (910256) ----------------------------------------------------------------------------------------------------------------
# Fold modes: 1 = norm, 5 = norm + write-back, 7 = norm + residual + write-back.  "Norm + residual" WITHOUT write-back (mode 3) cannot be reached in the forward form: the
# planner writes a normalised tensor back whenever it carries a residual (net_plan.hip, norm_folds: wb = res || consumers != 1) and launch_rb_fold instantiates no mode 3
# there.  Mode 3 exists in the transposed form only: the norm_res cases of 960256 below.
RB256 = [
    ("reflect_2x44x60", dict(cin=256, cout=256, shape=(2, 44, 60), reflect=True)),                      # 24 patches, ragged in both directions (86 % useful)
    ("zero_relu_2x44x60", dict(cin=256, cout=256, shape=(2, 44, 60), relu=True)),
    ("whole_2x48x64_bn", dict(cin=128, cout=512, shape=(2, 48, 64), relu=True, bn=True)),              # whole patches, two column tiles, folded BatchNorm
    ("pool_odd_2x45x61", dict(cin=256, cout=256, shape=(2, 45, 61), relu=True, pool=True)),             # fused pool; odd size: the last row / column is dropped
    ("eight_wave_13x64x64", dict(cin=128, cout=256, shape=(13, 64, 64), reflect=True)),                 # 208 patches >= 192: the eight-wave form itself
    ("norm_c128_8x60x64", dict(cin=128, cout=256, shape=(8, 60, 64), reflect=True, norm="relu")),       # folded norm (mode 1), ragged rows
    ("norm_c256_8x60x64", dict(cin=256, cout=256, shape=(8, 60, 64), reflect=True, norm="relu")),
    ("norm_wb_c256_8x60x64", dict(cin=256, cout=256, shape=(8, 60, 64), reflect=True, norm="wb")),      # ... with write-back (mode 5)
    ("norm_res_wb_c128_8x60x64", dict(cin=128, cout=256, shape=(8, 60, 64), reflect=True, norm="res")),  # norm + residual + write-back (mode 7)
    ("norm_res_wb_c256_8x64x64", dict(cin=256, cout=256, shape=(8, 64, 64), reflect=True, norm="res")),
    ("stats_c256_8x64x64", dict(cin=256, cout=256, shape=(8, 64, 64), reflect=True, stats=True)),       # statistics epilogue
    ("norm_stats_c256_8x64x64", dict(cin=256, cout=256, shape=(8, 64, 64), reflect=True, norm="relu", stats=True)),
]


@pytest.mark.parametrize("case", RB256, ids=_id)
def test_conv3x3_halo_rb_256_columns(cuda_device, case):
    _run(cuda_device, variant=910256, label="910256 " + case[0], **case[1])


# ---- conv3x3_halo.hip (9000xx): what conv3x3_halo_rb.hip refuses ------------------------------------------------------------------------------------------------------
HALO = [
    ("900064_stats_8x64x64", 900064, dict(cin=64, cout=64, shape=(8, 64, 64), reflect=True, stats=True)),         # the four-wave forms take no statistics
    ("900128_stats_8x64x64", 900128, dict(cin=128, cout=128, shape=(8, 64, 64), reflect=True, stats=True)),
    ("900128_cout320_2x44x60", 900128, dict(cin=64, cout=320, shape=(2, 44, 60), reflect=True, relu=True)),       # CoutPad 384: a multiple of 128, not of 256; 64 padded columns
    ("900064_tall_patch_rule_2x48x64", 900064, dict(cin=64, cout=64, shape=(2, 48, 64), relu=True)),              # 48 / 64 rows of the tall patches used: < 85 %
    ("900256_norm_c64_8x64x64", 900256, dict(cin=64, cout=256, shape=(8, 64, 64), reflect=True, norm="relu")),    # folded norm at Cin 64
]


@pytest.mark.parametrize("case", HALO, ids=_id)
def test_conv3x3_halo_lds_resident(cuda_device, case):
    _run(cuda_device, variant=case[1], label=case[0], **case[2])


# ---- conv_igemm_rb.hip (9402xx / 940128 / 940064) ---------------------------------------------------------------------------------------------------------------------
IRB = [
    ("940064_s2_c64_16x128x128", 940064, dict(cin=64, cout=64, shape=(16, 128, 128), stride=2, relu=True)),                 # 256 tiles of 256 rows
    ("940128_s2_c64_bn_16x127x129", 940128, dict(cin=64, cout=128, shape=(16, 127, 129), stride=2, relu=True, bn=True)),    # odd input: ragged last tile
    ("940256_s2_c128_16x128x128", 940256, dict(cin=128, cout=256, shape=(16, 128, 128), stride=2)),
    ("940064_dilated_c64_4x128x130", 940064, dict(cin=64, cout=64, shape=(4, 128, 130), dilation=2, relu=True)),            # RCF conv5 form
    ("940128_norm_s2_c64_16x128x128", 940128, dict(cin=64, cout=128, shape=(16, 128, 128), stride=2, norm="relu")),         # producer's norm folded in
    ("940128_stats_s2_c64_16x128x128", 940128, dict(cin=64, cout=128, shape=(16, 128, 128), stride=2, stats=True)),         # statistics epilogue
    ("940256_residual_1x1_s2_c128_16x128x128", 940256, dict(cin=128, cout=256, shape=(16, 128, 128), k=1, stride=2, residual=True, relu=True)),
    ("940256_transposed_norm_8x66x128", 940256, dict(cin=128, cout=64, shape=(8, 66, 128), transposed=True, stride=2, norm="relu")),   # 82 % useful area: the patch form refuses
]


@pytest.mark.parametrize("case", IRB, ids=_id)
def test_conv_igemm_rb(cuda_device, case):
    _run(cuda_device, variant=case[1], label=case[0], **case[2])


# ---- conv3x3_halo_rb.hip, transposed form (960256) ----------------------------------------------------------------------------------------------------------------------
CT = [
    ("plain_128to64_8x64x64", dict(cin=128, cout=64, shape=(8, 64, 64))),
    ("plain_256to128_ragged_4x60x64", dict(cin=256, cout=128, shape=(4, 60, 64))),                       # 94 % useful area, 64 patches x 2 column tiles
    ("stats_128to64_8x64x64", dict(cin=128, cout=64, shape=(8, 64, 64), stats=True)),
    ("stats_256to128_4x64x64", dict(cin=256, cout=128, shape=(4, 64, 64), stats=True)),
    ("norm_128to64_ragged_8x60x64", dict(cin=128, cout=64, shape=(8, 60, 64), norm="relu")),
    ("norm_stats_256to128_4x64x64", dict(cin=256, cout=128, shape=(4, 64, 64), norm="relu", stats=True)),
    ("norm_res_256to128_4x64x64", dict(cin=256, cout=128, shape=(4, 64, 64), norm="res", stats=True)),
    ("norm_res_128to64_ragged_8x60x64", dict(cin=128, cout=64, shape=(8, 60, 64), norm="res")),
]


@pytest.mark.parametrize("case", CT, ids=_id)
def test_transposed_conv_patch_form(cuda_device, case):
    _run(cuda_device, variant=960256, transposed=True, stride=2, label="960256 " + case[0], **case[1])


# ---- conv_igemm.hip: the generic tiles ----------------------------------------------------------------------------------------------------------------------------------
GENERIC = [
    ("256256_1x1_c32_8x128x128", 256256, dict(cin=32, cout=256, shape=(8, 128, 128), k=1, relu=True)),           # M = 131072: 512 tiles of 256 rows
    ("256128_1x1_c32_bn_8x128x128", 256128, dict(cin=32, cout=128, shape=(8, 128, 128), k=1, bn=True)),
    ("256064_1x1_c16_16x128x128", 256064, dict(cin=16, cout=64, shape=(16, 128, 128), k=1, relu=True)),           # 1024 tiles
    ("128128_3x3_c32_2x113x111", 128128, dict(cin=32, cout=128, shape=(2, 113, 111), reflect=True, relu=True)),   # 196 tiles of 128 rows, the last one ragged
    ("128064_3x3_c32_3x13x17", 128064, dict(cin=32, cout=64, shape=(3, 13, 17), reflect=True)),
    ("128032_3x3_c16_2x20x28", 128032, dict(cin=16, cout=32, shape=(2, 20, 28), relu=True)),
    ("128064_underfilled_c32_2x20x28", 128064, dict(cin=32, cout=128, shape=(2, 20, 28), relu=True, bn=True)),    # 9 tiles x 1 column tile < 192: 64-column tiles
    ("128064_s2_c32_residual_1x9x11", 128064, dict(cin=32, cout=64, shape=(1, 9, 11), stride=2, residual=True, relu=True)),
    ("256128_norm_s2_c64_2x64x64", 256128, dict(cin=64, cout=128, shape=(2, 64, 64), stride=2, norm="relu")),    # folded norm: too few tiles for conv_igemm_rb.hip
    ("128064_norm_s2_c64_2x64x64", 128064, dict(cin=64, cout=64, shape=(2, 64, 64), stride=2, norm="relu", relu=True)),
    ("128032_norm_s2_c64_2x64x64", 128032, dict(cin=64, cout=32, shape=(2, 64, 64), stride=2, norm="relu")),
]


@pytest.mark.parametrize("case", GENERIC, ids=_id)
def test_generic_implicit_gemm_tiles(cuda_device, case):
    _run(cuda_device, variant=case[1], label=case[0], **case[2])


# ---- conv_stem.hip (950049 / 950009): reflect stems and a resized stride-2 stem -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,stride,reflect,shape,scale,variant", [
    (7, 1, True, (4, 128, 128), None, 950049),
    (7, 1, True, (3, 150, 171), None, 950049),             # ragged tiles
    (3, 1, True, (4, 128, 128), None, 950009),
    (3, 1, True, (3, 150, 171), None, 950009),
    (7, 2, False, (2, 530, 531), 2 ** -0.5, 950049),       # ResNet stem through a resized call: 374 x 375 -> 187 x 188
])
def test_image_stem_general_forms(cuda_device, k, stride, reflect, shape, scale, variant):
    from gandtr_amd.engine import HipNet
    net = HipNet(cuda_device)
    t = net.input(3)
    wt, bias = synth._normal(0, "ws", (64, 3, k, k), math.sqrt(2.0 / (3 * k * k))), synth._normal(0, "bs", (64,), 0.2)
    bnp = _bn(0, 64) if stride == 2 else None
    tap = net.output_nchw(net.conv(t, wt, bias, bn=bnp, stride=stride, pad=k // 2, reflect=reflect, relu=stride == 2))
    tap_in = net.output_nchw(t)
    net.finalize()
    x = synth.synth_input(4, shape[:1] + (3,) + shape[1:]).to(cuda_device)
    net.set_profiling(True)
    outs = [o.cpu() for o in net.forward(x, scale=scale)]
    torch.cuda.synchronize()
    variants = _conv_variants(net)
    net.set_profiling(False)
    again = net.forward(x, scale=scale)
    xin = outs[tap_in][:, :3]
    assert torch.equal(cb.f16(xin), xin)
    wp, shift = cb.fold(wt, bias, bnp)
    label = "%d k%d s%d %s" % (variant, k, stride, shape)
    print("%s: variants %s" % (label, variants))
    cb.assert_layer(outs[tap], xin, wp, shift, label, stride=stride, pad=k // 2, reflect=reflect, act="relu" if stride == 2 else None)
    got, r = outs[tap][:1], cb.layer(xin[:1], wp, shift, stride=stride, pad=k // 2, reflect=reflect, act="relu" if stride == 2 else None)
    for sl in ((0, slice(None), 0), (0, slice(None), -1), (0, slice(None), slice(None), 0), (0, slice(None), slice(None), -1)):      # image borders
        assert bool(((got[sl].double() - r.ref[sl]).abs() <= r.bound[sl]).all())
    assert variants[0] == variant, variants
    assert all(torch.equal(p, q.cpu()) for p, q in zip(outs, again))
