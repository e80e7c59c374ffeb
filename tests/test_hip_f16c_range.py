"""The f16c precision contract across activation MAGNITUDES.

Every other compensated-conv test feeds O(1) activations.  The correction product of the f16c mode stores the activation residuals as
e2m1 (fp4: {0, 0.5, 1, 1.5, 2, 3, 4, 6}) under an E8M0 scale, so how that scale is chosen decides whether the correction survives
activations that are much larger or smaller than 1 (residual streams, BatchNorm nets, trained checkpoints).  Here each compensated form
runs the same layer on inputs scaled by 2^s:
  (a) the layer's own gate against fp64 holds at every scale;
  (b) the error is flat: err(s) <= 1.5 err(0);
  (c) exact equivariance: with |a| in [2^-3, 2^3] u {0} and no bias, out(2^s x) == 2^s out(x) bit for bit.  Products of fp16 values
      accumulated in fp32 are exactly equivariant, and so is a block-scaled product whose scales follow the data; the single-pass "f16"
      mode runs the same layers as the control.
and a BatchNorm generator, rescaled so that the function stays the same while every hidden activation is multiplied by c, holds the
1e-3 contract at every c.
Uniform scaling cannot see WHICH pixel's scale a fragment uses, so the same layers also run on magnitudes spread over 2^+-6 from pixel to
pixel and over 2^+-3 from channel to channel.
Measured before the activation side of the correction took a per-pixel scale (fixed 2^12 for a_lo, 1 for a_hi): every compensated form,
the head's included, left the 2e-4 gate outside about [2^-2, 2^2] (c16 2.7e-4 at 2^-8, 6.6e-5 at 1, 2.7e-4 at 2^8; f16ch head 3.3e-4 /
4.7e-5 / 3.2e-4) -- it fell back to single-pass fp16."""
import pytest
import torch
import torch.nn.functional as F

from gandtr_amd.engine import HipNet, build_generator
from gandtr_amd.tools import synth
from oracle import gandtr_oracle as O

pytestmark = pytest.mark.gpu

SWEEP = (-8, -4, -2, 0, 2, 4, 8)
EXACT = tuple(range(-6, 7))


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _g(seed, name, shape, std=1.0):
    return synth._normal(seed, name, shape, std)


# name: (cin, cout, n, h, w, conv kwargs, kernel variant that must run the layer in f16c, gate against fp64).  h, w: the INPUT size.
FORMS = {
    "c16": (256, 256, 16, 64, 64, dict(pad=1, reflect=True), 971256, 2e-4),             # conv3x3_halo_c16, whole patches
    "c128": (256, 256, 8, 64, 64, dict(pad=1, reflect=True), 970128, 2e-4),             # conv3x3_halo_c, 128 columns
    "c256_ragged": (256, 256, 8, 76, 92, dict(pad=1), 970256, 2e-4),                    # conv3x3_halo_c, 256 columns (240 tiles), ragged grid
    "s2_128_256": (128, 256, 8, 128, 128, dict(stride=2, pad=1), 990256, 2e-4),         # FORM 2
    "s2_64_128": (64, 128, 8, 128, 128, dict(stride=2, pad=1), 990256, 2e-4),
    "ct_256_128": (256, 128, 8, 64, 64, dict(stride=2, pad=1, transposed=True), 980256, 3e-4),     # FORM 1 (test_halo_c_transposed's gate)
    "ct_128_64": (128, 64, 8, 64, 64, dict(stride=2, pad=1, transposed=True), 980256, 3e-4),
}


def _ref_conv(a, wt, kw):
    if kw.get("transposed"):
        return F.conv_transpose2d(a, wt.double(), stride=2, padding=1, output_padding=1)
    if kw.get("reflect"):
        return F.conv2d(F.pad(a, (1,) * 4, mode="reflect"), wt.double())
    return F.conv2d(a, wt.double(), stride=kw.get("stride", 1), padding=kw.get("pad", 0))


def _weights(form):
    cin, cout, n, h, w, kw, variant, gate = FORMS[form]
    return _g(0, "w", (cin, cout, 3, 3) if kw.get("transposed") else (cout, cin, 3, 3), 0.05)


def _forward(net, x, dev):
    net.set_profiling(True)
    outs = net.forward(x.to(dev))
    torch.cuda.synchronize()
    return outs, [v for k, v, ms, fl in net.profile() if k == 1]


def _check_sweep(errs, gate, what):
    """(a) the gate at every scale, (b) flat in the scale; every number in the message"""
    table = "  ".join("2^%+d: %.2e" % (s, e) for s, e in errs.items())
    print("%s: %s" % (what, table))
    bad_gate = [s for s, e in errs.items() if not e < gate]
    bad_flat = [s for s, e in errs.items() if not e <= 1.5 * errs[0]]
    assert not bad_gate and not bad_flat, "%s: gate %.0e broken at 2^%s, not flat (> 1.5 err(0)) at 2^%s -- %s" % (what, gate, bad_gate, bad_flat, table)


@pytest.mark.parametrize("form", list(FORMS))
def test_compensated_conv_activation_scale_sweep(cuda_device, form):
    """3x3 / stride-2 / transposed compensated convs on activations 2^s * O(1) (a 1x1 prologue of the image, the input scaled by 2^s):
    the layer's gate against fp64 at every scale, and an error that does not depend on the scale"""
    cin, cout, n, h, w, kw, variant, gate = FORMS[form]
    net = HipNet(cuda_device, "f16c")
    t0 = net.conv(net.input(3), _g(0, "w0", (cin, 3, 1, 1), 0.7))
    wt = _weights(form)
    tap = net.output_nchw(net.conv(t0, wt, None, **kw))
    net.finalize()
    x = synth.synth_input(1, (n, 3, h, w))
    ref = _ref_conv(F.conv2d(x.double(), _g(0, "w0", (cin, 3, 1, 1), 0.7).double()), wt, kw)      # homogeneous: ref(2^s x) = 2^s ref(x)
    errs = {}
    for s in SWEEP:
        outs, ran = _forward(net, x * 2.0 ** s, cuda_device)
        assert variant in ran, (form, ran)
        errs[s] = _rel(outs[tap].double().cpu(), ref * 2.0 ** s)
    _check_sweep(errs, gate, form)


@pytest.mark.parametrize("n", [8, 16])
def test_compensated_conv_residual_stream_scale_sweep(cuda_device, n):
    """MODE 2 staging y = x + IN(conv) -> 3x3 conv: the ResnetBlock's residual stream.  IN(.) is O(1) whatever its input; the residual x
    carries the magnitude of the stream (it grows block by block in a trained net), so only x is scaled: input channels 4-7 feed it"""
    c = 256
    net = HipNet(cuda_device, "f16c")
    xin = net.input(8)
    w0 = torch.cat([_g(0, "w0", (c, 4, 1, 1), 0.7), torch.zeros(c, 4, 1, 1)], 1)
    w1 = torch.cat([torch.zeros(c, 4, 1, 1), _g(0, "w1", (c, 4, 1, 1), 0.7)], 1)
    t0, r = net.conv(xin, w0), net.conv(xin, w1)
    t = net.instance_norm(t0, relu=False, residual=r)
    wt = _g(0, "w", (c, c, 3, 3), 0.05)
    tap = net.output_nchw(net.conv(t, wt, None, pad=1, reflect=True))
    net.finalize()
    x = synth.synth_input(3, (n, 8, 64, 64))
    a0 = F.instance_norm(F.conv2d(x.double(), w0.double()), eps=1e-5)
    errs = {}
    for s in SWEEP:
        xs = x.clone()
        xs[:, 4:] *= 2.0 ** s
        outs, ran = _forward(net, xs, cuda_device)
        assert 971256 in ran if n == 16 else 970128 in ran, ran
        ref = F.conv2d(F.pad(a0 + F.conv2d(xs.double(), w1.double()), (1,) * 4, mode="reflect"), wt.double())
        errs[s] = _rel(outs[tap].double().cpu(), ref)
    _check_sweep(errs, 2e-4, "x + IN(conv), n = %d" % n)


@pytest.mark.parametrize("n", [8, 16])
def test_compensated_conv_bn_epilogue_residual_scale_sweep(cuda_device, n):
    """the BatchNorm generator's second ResnetBlock conv y = x + BN(conv(pad(x))) (test_halo_c_conv3x3_epilogue_residual) on x * 2^s,
    with the BatchNorm's mean and shift scaled alike (the layer is then homogeneous: ref(2^s x) = 2^s ref(x))"""
    c = 256
    x = synth.synth_input(2, (n, 3, 64, 64))
    wt = _g(0, "w", (c, c, 3, 3), 0.05)
    g, be, m, v = 1.0 + _g(0, "g", (c,), 0.2), _g(0, "be", (c,), 0.2), _g(0, "m", (c,), 0.3), 0.5 + _g(0, "v", (c,), 0.1).abs()
    a0 = F.conv2d(x.double(), _g(0, "w0", (c, 3, 1, 1), 0.7).double())
    ref = a0 + F.batch_norm(F.conv2d(F.pad(a0, (1,) * 4, mode="reflect"), wt.double()), m.double(), v.double(), g.double(), be.double(), False, 0.0, 1e-5)
    errs = {}
    for s in SWEEP:
        k = 2.0 ** s
        net = HipNet(cuda_device, "f16c")
        t0 = net.conv(net.input(3), _g(0, "w0", (c, 3, 1, 1), 0.7))
        tap = net.output_nchw(net.conv(t0, wt, None, bn=(g, be * k, m * k, v), pad=1, reflect=True, residual=t0))
        net.finalize()
        outs, ran = _forward(net, x * k, cuda_device)
        assert 971256 in ran or 970256 in ran if n == 16 else 970128 in ran, ran
        errs[s] = _rel(outs[tap].double().cpu(), ref * k)
    _check_sweep(errs, 2e-4, "x + BN(conv(x)), n = %d" % n)


def _head_net(dev, precision):
    net = HipNet(dev, precision)
    t0 = net.conv(net.input(3), _g(0, "w0", (64, 3, 1, 1), 0.7))
    slot = net.conv(t0, _g(0, "w", (3, 64, 7, 7), 0.02), None, pad=3, reflect=True, out_f32=True, act=0)
    net.finalize()
    return net, slot


@pytest.mark.parametrize("precision,gate", [("f16ch", 2e-4), ("f16c", 6e-4)])
def test_head7_activation_scale_sweep(cuda_device, precision, gate):
    """the generator head (ReflectionPad2d(3) + Conv2d(64, 3, 7), conv_head7.hip) on activations 2^s * O(1): its compensated MX form
    ("f16ch") at the compensated gate, the default single-pass form at test_head7_f32_input's 6e-4 (a regression guard: it has no
    correction product, so it should not depend on the scale at all)"""
    net, slot = _head_net(cuda_device, precision)
    x = synth.synth_input(7, (4, 3, 128, 160))
    a = F.conv2d(x.double(), _g(0, "w0", (64, 3, 1, 1), 0.7).double())
    ref = F.conv2d(F.pad(a, (3,) * 4, mode="reflect"), _g(0, "w", (3, 64, 7, 7), 0.02).double())
    errs = {}
    for s in SWEEP:
        outs, ran = _forward(net, x * 2.0 ** s, cuda_device)
        assert 920007 in ran, ran
        errs[s] = _rel(outs[slot].double().cpu(), ref * 2.0 ** s)
    _check_sweep(errs, gate, "head7 " + precision)


def test_stem_activation_scale_sweep(cuda_device):
    """regression guard: the f16c stem (fp16 pixel words augmented with their own rounding residuals, test_stem_c) on images 2^s * O(1)"""
    net = HipNet(cuda_device, "f16c")
    w = _g(0, "w", (64, 3, 7, 7), 0.1)
    slot = net.output_nchw(net.conv(net.input(3), w, None, pad=3, reflect=True))
    net.finalize()
    x = synth.synth_input(5, (4, 3, 256, 256), 1.0)
    ref = F.conv2d(F.pad(x.double(), (3,) * 4, mode="reflect"), w.double())
    errs = {}
    for s in SWEEP:
        outs, _ = _forward(net, x * 2.0 ** s, cuda_device)
        errs[s] = _rel(outs[slot].double().cpu(), ref * 2.0 ** s)
    _check_sweep(errs, 1e-5, "stem f16c")


def _spread(kind, x, w0):
    """magnitudes that differ from pixel to pixel (each input pixel times 2^k, k uniform in -6 .. 6: the 1x1 prologue keeps the factor) or
    from channel to channel (prologue output channel c times 2^k_c, k_c uniform in -3 .. 3)"""
    gen = torch.Generator().manual_seed(13)
    if kind == "pixel":
        k = torch.randint(-6, 7, (x.shape[0], 1, x.shape[2], x.shape[3]), generator=gen).float()
        return x * 2.0 ** k, w0
    k = torch.randint(-3, 4, (w0.shape[0], 1, 1, 1), generator=gen).float()
    return x, w0 * 2.0 ** k


@pytest.mark.parametrize("kind", ["pixel", "channel"])
@pytest.mark.parametrize("form", list(FORMS) + ["head"])
def test_compensated_conv_spread_magnitudes(cuda_device, form, kind):
    """every compensated form (the head: its "f16ch" MX form) on activations whose magnitude varies by 2^12 between neighbouring pixels, or
    by 2^6 between channels, against fp64 at the form's gate: a fragment that took the scale of another pixel (or of another stage) saturates
    or loses its correction there"""
    if form == "head":
        cin, n, h, w, kw, variant, gate = 64, 4, 128, 160, None, 920007, 2e-4
        wt = _g(0, "w", (3, 64, 7, 7), 0.02)
    else:
        cin, cout, n, h, w, kw, variant, gate = FORMS[form]
        wt = _weights(form)
    x, w0 = _spread(kind, synth.synth_input(1, (n, 3, h, w)), _g(0, "w0", (cin, 3, 1, 1), 0.7))
    net = HipNet(cuda_device, "f16ch" if form == "head" else "f16c")
    t0 = net.conv(net.input(3), w0)
    if form == "head":
        slot = net.conv(t0, wt, None, pad=3, reflect=True, out_f32=True, act=0)
    else:
        slot = net.output_nchw(net.conv(t0, wt, None, **kw))
    net.finalize()
    outs, ran = _forward(net, x, cuda_device)
    assert variant in ran, (form, ran)
    a = F.conv2d(x.double(), w0.double())
    ref = F.conv2d(F.pad(a, (3,) * 4, mode="reflect"), wt.double()) if form == "head" else _ref_conv(a, wt, kw)
    err = _rel(outs[slot].double().cpu(), ref)
    print("%s, spread over %ss: %.2e" % (form, kind, err))
    assert err < gate, err


def _exact_input(n, h, w):
    """8 channels, |x| in [2^-2, 2^2) u {0}, 21-bit mantissas: every split and product below is exact at every scale 2^s, |s| <= 6"""
    gen = torch.Generator().manual_seed(11)
    mant = 1.0 + torch.randint(0, 1 << 20, (n, 8, h, w), generator=gen).double() / (1 << 20)
    ex = torch.randint(-2, 2, (n, 8, h, w), generator=gen).double()
    sign = torch.randint(0, 2, (n, 8, h, w), generator=gen).double() * 2 - 1
    keep = (torch.rand((n, 8, h, w), generator=gen) > 0.1).double()
    return (sign * mant * 2.0 ** ex * keep).float()


def _selection(cin):
    """1x1 weights 8 -> cin with ONE entry +-2^g per output channel (g in {-1, 0, 1}): the conv input is 2^g * x[c % 8] exactly"""
    gen = torch.Generator().manual_seed(12)
    w = torch.zeros(cin, 8, 1, 1)
    gexp = torch.randint(-1, 2, (cin,), generator=gen).float()
    sign = torch.randint(0, 2, (cin,), generator=gen).float() * 2 - 1
    w[torch.arange(cin), torch.arange(cin) % 8, 0, 0] = sign * 2.0 ** gexp
    return w


def _exact_case(dev, precision, form):
    if form == "head":
        cin, n, h, w = 64, 4, 128, 160
    else:
        cin, cout, n, h, w, kw, variant, gate = FORMS[form]
    net = HipNet(dev, precision)
    t0 = net.conv(net.input(8), _selection(cin))
    tin = net.output_nchw(t0)
    if form == "head":
        out = net.conv(t0, _g(0, "w", (3, 64, 7, 7), 0.02), None, pad=3, reflect=True, out_f32=True, act=0)
    else:
        out = net.output_nchw(net.conv(t0, _weights(form), None, **kw))
    net.finalize()
    return net, tin, out, _exact_input(n, h, w)


@pytest.mark.parametrize("form,precision", [(f, p) for f in FORMS for p in ("f16c", "f16")]
                         + [("head", "f16c"), ("head", "f16")])
def test_conv_exactly_equivariant_under_power_of_two_scaling(cuda_device, form, precision):
    """(c): the layer's output at 2^s x is 2^s times its output at x, bit for bit, for s in -6 .. 6 -- in the compensated modes (the
    head: its "f16ch" MX form) and in single-pass fp16, the control.  The conv input is checked to scale exactly first.
    The control stores its output in fp16, where outputs below 2^-14 are subnormal and round to a fixed grid (measured on the device: only
    those differ, by <= 6e-8 of max|out| at 2^-6): it is compared where |out(x)| >= 2^-8, normal at every scale.  The compensated modes
    write fp32 and are compared everywhere."""
    if form == "head" and precision == "f16c":
        precision = "f16ch"
    net, tin, out, x = _exact_case(cuda_device, precision, form)
    outs, ran = _forward(net, x, cuda_device)
    if precision != "f16":
        assert (920007 if form == "head" else FORMS[form][6]) in ran, ran
    a1, y1 = outs[tin].clone(), outs[out].clone()
    keep = (y1.abs() >= 2.0 ** -8) if precision == "f16" else torch.ones_like(y1, dtype=torch.bool)
    assert float(a1.abs().max()) <= 8 and float(a1[a1 != 0].abs().min()) >= 0.125
    bad = []
    for s in EXACT:
        outs, _ = _forward(net, x * 2.0 ** s, cuda_device)
        assert torch.equal(outs[tin], a1 * 2.0 ** s), s            # precondition: the conv's input is exactly 2^s times
        if not torch.equal(outs[out][keep], y1[keep] * 2.0 ** s):
            bad.append((s, float(((outs[out] - y1 * 2.0 ** s).abs().max() / (y1.abs().max() * 2.0 ** s)))))
    assert not bad, "%s %s: out(2^s x) != 2^s out(x) at (s, max|d| / max|out|) %s" % (form, precision, bad)


# ---- the whole generator: a BatchNorm ResnetGenerator rescaled so that its function stays the same while every hidden activation is c times larger

TAPS = (1, 3, 9, 10, 14, 18, 21, 24, 26)


def _head_scaled(sd, x, target):
    """test_hip_models.py::_head_scaled: the head scaled so that max|pre-tanh| on x is `target` (the image spans the tanh's working range)"""
    _, f = O.resnet_generator(x, sd, "batch", 9, taps=(26,))
    k = target / float(f[26].abs().max())
    sd = dict(sd)
    sd["model.26.weight"] = sd["model.26.weight"] * k
    sd["model.26.bias"] = sd["model.26.bias"] * k
    return sd


def _rescaled(sd, c, eps=1e-5):
    """every hidden activation times c, the same function: the convs before the head have no bias and ReLU, reflection pad, residual adds and
    convs are homogeneous, so it is enough to scale every BatchNorm's output by c and the head's weights by 1 / c"""
    sd = dict(sd)
    assert all(k == "model.26.bias" or k[:-len("bias")] + "running_mean" in sd for k in sd if k.endswith(".bias"))
    for k in [k for k in sd if k.endswith(".running_mean")]:
        p = k[:-len("running_mean")]
        if p == "model.2.":           # the first BatchNorm: its input keeps its magnitude, its normalisation takes the factor
            sd[p + "running_var"] = (sd[p + "running_var"] + eps) / (c * c) - eps
        else:
            sd[p + "running_mean"] = sd[p + "running_mean"] * c
        sd[p + "bias"] = sd[p + "bias"] * c
    sd["model.26.weight"] = sd["model.26.weight"] / c
    return sd


@pytest.fixture(scope="module")
def bn_generator():
    x = synth.synth_input(2, (8, 3, 256, 256), 1.0)
    base = {}

    def get(target):
        if target not in base:
            sd = _head_scaled(synth.generator_state(0, "batch"), x, target)
            base[target] = (sd,) + O.resnet_generator(x, sd, "batch", 9, taps=TAPS)
        return base[target]
    return x, get


@pytest.mark.parametrize("precision,c", [("f16c", 1 / 16), ("f16c", 1 / 4), ("f16c", 1.0), ("f16c", 4.0), ("f16c", 16.0), ("f16ch", 16.0)])
def test_generator_contract_at_scaled_activations(cuda_device, bn_generator, precision, c):
    """BatchNorm generator (batch 8 x 256^2) with every hidden activation c times larger and the same function: every tap and the
    pre-tanh output within 1e-3 of the oracle on the rescaled weights, the pre-tanh output within 1e-3 of the c = 1 oracle, and the
    image gates of test_generator_image_absolute_gate (max|pre-tanh| 1.5 for f16c, 3 for the compensated head)"""
    x, get = bn_generator
    target = 3.0 if precision == "f16ch" else 1.5
    sd1, ref1, feats1 = get(target)
    sd = _rescaled(sd1, c)
    ref, feats = O.resnet_generator(x, sd, "batch", 9, taps=TAPS)
    assert _rel(feats[18], feats1[18] * c) < 1e-5 and _rel(feats[26], feats1[26]) < 1e-5      # the rescaling is what it claims to be
    net = build_generator(sd, cuda_device, taps=TAPS, precision=precision)
    outs = net.forward(x.to(cuda_device))
    rels = {t: _rel(outs[net.tap_slots[t]].cpu(), feats[t]) for t in TAPS}
    pre = outs[net.tap_slots[26]].cpu()
    d = (outs[net.out_slot].cpu() - ref1).abs().flatten()
    mx, p999, mean = float(d.max()), float(torch.quantile(d[::2], 0.999)), float(d.mean())
    print("%s c = %g: taps %s; pre-tanh vs c = 1: %.2e; image max %.2e p99.9 %.2e mean %.2e"
          % (precision, c, " ".join("%d:%.1e" % kv for kv in rels.items()), _rel(pre, feats1[26]), mx, p999, mean))
    assert all(r < 1e-3 for r in rels.values()), rels
    assert _rel(pre, feats1[26]) < (4e-4 if precision == "f16ch" else 1e-3)
    assert mx <= 1e-3 and p999 <= 7e-4 and mean <= 2e-4, (mx, p999, mean)
