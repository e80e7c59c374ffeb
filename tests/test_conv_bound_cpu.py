"""The per-output bound of tests/conv_bound.py against itself, on the CPU: the emulation of a correct kernel (fp32 accumulation, one fp16 store) stays under the bound
through every option of the helper, and the emulations of wrong kernels exceed it.

Measured (max |d| / bound): plain emulation 0.73 / 0.29 / 0.75 / 0.56 on the four shapes below; over all options 0.27 - 0.93, except the folded-norm options
(0.09 - 0.25: their bound carries the worst case of every input's fp16 rounding) and the fp32 tanh head (0.000 - 0.006: no fp16 store).  fp16 rounding between 64-wide K
chunks 3.1 / 4.4 and a shift added after the fp16 store 1.2 / 1.4 on the two K <= 576 shapes (the old gate sees 6e-4 .. 9e-4 of its 2e-3); one dropped product 23.5 / 1.7 /
13.2 / 7.3; zero for reflect padding on one edge of 8 channels 1068 / 95 / 4543."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_bound as cb
from gandtr_amd.tools import synth

# (cin, cout, k, n, h, w)
SHAPES = [(64, 64, 3, 1, 24, 40), (256, 256, 3, 1, 20, 36), (8, 64, 7, 1, 24, 40), (1024, 256, 1, 1, 16, 16)]
SMALL_K = [s for s in SHAPES if s[0] * s[2] * s[2] <= 576]
IDS = lambda s: "%dto%d_k%d" % s[:3]


def _data(shape, transposed=False, bn=False):
    cin, cout, k, n, h, w = shape
    a = cb.f16(synth._normal(11, "a", (n, cin, h, w), 0.8))
    wt = synth._normal(12, "w", (cin, cout, k, k) if transposed else (cout, cin, k, k), math.sqrt(2.0 / (cin * k * k)))
    bias = synth._normal(13, "b", (cout,), 0.2)
    bnp = None
    if bn:
        bnp = (synth._uniform(14, "g", (cout,), 0.5, 1.5), synth._normal(14, "be", (cout,), 0.2), synth._normal(14, "m", (cout,), 0.2), synth._uniform(14, "v", (cout,), 0.5, 1.5))
    wp, shift = cb.fold(wt, bias, bnp, transposed)
    return a, wp, shift


def _opts(shape):
    k = shape[2]
    return dict(pad=k // 2, reflect=k > 1)


OPTIONS = {
    "plain": {},
    "zero_pad": dict(reflect=False),
    "stride2": dict(stride=2, reflect=False),
    "dilated": dict(dilation=2, pad=None, reflect=False),
    "relu": dict(act="relu"),
    "leaky": dict(act="leaky", leaky=0.2),
    "tanh_f32": dict(act="tanh", out_f32=True),
    "bn": dict(bn=True, act="relu"),
    "residual": dict(residual=True),
    "residual_relu": dict(residual=True, act="relu"),
    "pool": dict(act="relu", pool=True),
    "transposed": dict(transposed=True),
    "transposed_bn": dict(transposed=True, bn=True),
    "norm": dict(norm=True),
    "norm_residual": dict(norm="res"),
}


def _case(shape, name):
    """(input, packed weights, shift, layer() / emulate() keywords, what emulate() stages) of one option on one shape"""
    o = dict(OPTIONS[name])
    transposed, bn, norm = o.pop("transposed", False), o.pop("bn", False), o.pop("norm", False)
    a, wp, shift = _data(shape, transposed, bn)
    kw = dict(transposed=True) if transposed else _opts(shape)
    kw.update(o)
    if kw.get("pad", 0) is None:
        kw["pad"] = 2 * (shape[2] // 2)
    cin, cout, k, n, h, w = shape
    if kw.pop("residual", False):
        probe = cb.layer(a, wp, shift, **kw)
        kw["residual"] = cb.f16(synth._normal(15, "r", tuple(probe.ref.shape), 0.8))
    stage = None
    if norm:                                        # the conv folds InstanceNorm + ReLU (or InstanceNorm + residual) of the tensor x into its staging
        x = cb.f16(synth._normal(16, "x", tuple(a.shape), 1.3) + 0.4)
        res = cb.f16(synth._normal(17, "xr", tuple(a.shape), 0.8)) if norm == "res" else None
        mean, rstd = cb.emulate_stats(x)            # the device's statistics: fp32 partial sums
        z = x * rstd.float()[:, :, None, None] - (mean * rstd).float()[:, :, None, None]
        stage = cb.f16(F.relu(z) if res is None else z + res)
        a, kw["in_delta"] = cb.norm_input(x, relu=res is None, residual=res)
    return a, wp, shift, kw, stage


# (the transposed form is k3 s2 p1 op1: the two 3 x 3 shapes)
CASES = [(s, n) for s in SHAPES for n in OPTIONS if s[2] == 3 or not OPTIONS[n].get("transposed")]


@pytest.mark.parametrize("shape,name", CASES, ids=lambda v: IDS(v) if isinstance(v, tuple) else v)
def test_emulation_stays_under_its_bound(shape, name):
    a, wp, shift, kw, stage = _case(shape, name)
    r = cb.layer(a, wp, shift, **kw)
    ekw = {k: v for k, v in kw.items() if k != "in_delta"}
    got = cb.emulate(a, wp, shift, in_stage=stage, **ekw)
    assert cb.assert_within(got, r, "%s %s" % (IDS(shape), name)) > 0.0


@pytest.mark.parametrize("fault", ["chunk16", "bias_late"])
@pytest.mark.parametrize("shape", SMALL_K, ids=IDS)
def test_rounding_faults_exceed_the_bound(shape, fault):
    """an accumulator that passes through fp16 between K chunks, a value rounded twice: the global gate max|d| / max|ref| < 2e-3 sees neither"""
    a, wp, shift = _data(shape)
    kw = _opts(shape)
    r = cb.layer(a, wp, shift, **kw)
    q, pos, rel = cb.ratio(cb.emulate(a, wp, shift, fault=fault, **kw), r)
    print("%s %s: max |d| / bound = %.2f at %s; max|d| / max|ref| = %.2e" % (IDS(shape), fault, q, pos, rel))
    assert q > 1.0
    assert rel < 2e-3


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_a_dropped_product_exceeds_the_bound(shape):
    """one product missing at one border pixel (the top-left output, centre tap, the channel of median |a w|)"""
    a, wp, shift = _data(shape)
    kw = _opts(shape)
    r = cb.layer(a, wp, shift, **kw)
    got = cb.emulate(a, wp, shift, **kw)
    c = shape[2] // 2
    prods = a[0, :, 0, 0].double() * wp[5, :, c, c]
    ch = int(torch.argsort(prods.abs())[len(prods) // 2])
    got[0, 5, 0, 0] = cb.f16(got[0, 5, 0, 0] - prods[ch].float())
    q, pos, rel = cb.ratio(got, r)
    print("%s: dropped product %.3e: max |d| / bound = %.1f at %s" % (IDS(shape), float(prods[ch]), q, pos))
    assert q > 1.0 and pos == (0, 5, 0, 0)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[2] > 1], ids=IDS)
def test_zero_for_reflect_padding_exceeds_the_bound(shape):
    """zero padding in place of reflect padding above the top edge, for 8 of the input channels"""
    a, wp, shift = _data(shape)
    kw = _opts(shape)
    r = cb.layer(a, wp, shift, **kw)
    p = kw["pad"]
    padded = F.pad(a, (p,) * 4, mode="reflect")
    padded[:, :8, :p, :] = 0
    got = cb.emulate(padded, wp, shift, pad=0)
    q, pos, rel = cb.ratio(got, r)
    print("%s: max |d| / bound = %.1f at %s" % (IDS(shape), q, pos))
    assert q > 1.0 and pos[2] < p


# (cin, (n, h, w)) of the tensors behind a folded norm in tests/test_hip_layer_bounds.py and tests/test_hip_layers.py: the 1 x 1 lift of a synthetic image
NORM_SHAPES = [(128, (8, 60, 64)), (256, (8, 60, 64)), (256, (8, 64, 64)), (64, (16, 128, 128)), (64, (2, 64, 64)), (128, (8, 66, 128)), (256, (4, 64, 64)),
               (128, (8, 64, 64)), (64, (8, 64, 64))]


def test_statistics_error_is_the_measured_one():
    """the one measured term of the bound (conv_bound.STAT_ERR_R / STAT_ERR_M): the device's InstanceNorm statistics, emulated (fp32 partial sums over 128 rows of the
    fp32 values before the fp16 store, as a conv epilogue takes them; over 32 rows; over 128 and 4096 rows of the stored fp16 tensor, as the separate pass does) against
    float64 statistics of the fp16 tensor, on the shapes of the GPU tests.  The allowance is twice the largest value: this prints the values and holds them to half of it."""
    worst_r = worst_m = 0.0
    for cin, shape in NORM_SHAPES:
        x = synth.synth_input(1, (shape[0], 3) + shape[1:])
        pre = F.conv2d(cb.f16(x), cb.f16(synth._normal(0, "w0", (cin, 3, 1, 1), 0.7)))      # fp32 values before the store
        t = cb.f16(pre).double()                                                                # the tensor a test taps
        mean, rstd = t.mean(dim=(2, 3)), 1 / torch.sqrt(t.var(dim=(2, 3), unbiased=False) + 1e-5)
        for src, rows in ((pre, 128), (pre, 32), (cb.f16(pre), 128), (cb.f16(pre), 4096)):
            m2, r2 = cb.emulate_stats(src, rows)
            worst_r, worst_m = max(worst_r, float((r2 / rstd - 1).abs().max())), max(worst_m, float(((m2 - mean).abs() * rstd).max()))
    print("statistics error over %d shapes: e_r = %.3e, e_m = %.3e (allowed: %.1e, %.1e)" % (len(NORM_SHAPES), worst_r, worst_m, cb.STAT_ERR_R, cb.STAT_ERR_M))
    assert worst_r <= cb.STAT_ERR_R / 2 * 1.01 and worst_m <= cb.STAT_ERR_M / 2 * 1.01
