"""The patch conv kernels are BIT-EXACT under image translation.

The value of an output pixel depends on its input neighbourhood and the weights only -- not on where the pixel lies in its 16 x 16 patch,
which image of the batch it is in, which tile of a persistent workgroup's list computes it, or whether its neighbourhood was staged as halo
ring or as patch body.  By the kernels' code this holds bit for bit: every output element of a tile goes through the same MFMAs in the same
chunk / tap / k-substep order, the compensated mode splits an activation per pixel and 64-channel chunk (fp16 hi + fp4 residual under that
pixel's E8M0 scale, gdt_c_pixel_exp), and a zero-padded halo pixel contributes exact zeros.  The global gates of test_hip_f16c*.py (2e-4 of
max|ref|, against 5e-4 for single-pass fp16) say the correction product is there; they cannot see it missing at one tap, on the halo ring,
at patch seams, in a ragged tile's checked epilogue or in a workgroup's first tile (about 1.7e-4, locally).  This file can: one forward on
a batch whose images hold the same content at different places (tests/position_windows.py), torch.equal on the windows.  Nothing here has
a tolerance; a single differing bit fails, and the message says at which patch-relative positions and output channels.

Each case: HipNet, a bias-free 1 x 1 lift of a 3-channel image (zero pixels stay zero), the layer under test with a bias; one forward; the
kernel variant pinned through net.profile().  Every image of a batch has its own offset, so batch position and tile-list position vary too."""
import pytest
import torch

import position_windows as PW
from gandtr_amd.engine import HipNet
from gandtr_amd.tools import synth

pytestmark = pytest.mark.gpu


def _g(seed, name, shape, std=1.0):
    return synth._normal(seed, name, shape, std)


def _content(name, seed=3):
    pl = PW.PLACEMENTS[name]
    return _g(seed, "content", (3,) + tuple(pl["content"]), 1.0)


def _forward(net, batch, dev):
    net.set_profiling(True)
    outs = net.forward(batch.to(dev))
    torch.cuda.synchronize()
    return outs, [v for k, v, ms, fl in net.profile() if k == 1]


def _check(out, pairs, what):
    """all windows equal; the number of outputs compared and the coverage of the patch are printed and asserted"""
    rep = PW.compare(out, pairs)
    print("%s: %s" % (what, rep.summary()))
    assert rep.positions == 256 and rep.compared > 0, what
    assert rep.ok, "%s: the same neighbourhood gave other values at another place -- %s" % (what, rep.summary())


def _lifted_is_placed(out_lift, batch):
    """precondition: the lift of a zero pixel is zero and of a content pixel is not (the windows hold what they claim to hold)"""
    assert torch.equal(out_lift.cpu().abs().sum(1) != 0, batch.abs().sum(1) != 0)


def _layer_case(dev, precision, placement, cin, wt, kw, variant, what, bias=True, bn=None, residual=False, stats=False, seed=3):
    """``stats``: an InstanceNorm follows the layer (its statistics come from the layer's epilogue: another form of the kernel); its result is not compared"""
    batch, pairs = PW.place(placement, _content(placement, seed))
    net = HipNet(dev, precision)
    t0 = net.conv(net.input(3), _g(0, "w0", (cin, 3, 1, 1), 0.7))
    tin = net.output_nchw(t0)
    cout = wt.shape[1] if kw.get("transposed") else wt.shape[0]
    out = net.conv(t0, wt, _g(0, "b", (cout,), 0.2) if bias else None, bn=bn, residual=t0 if residual else -1, **kw)
    tap = out if kw.get("out_f32") else net.output_nchw(out)
    if stats:
        net.output_nchw(net.instance_norm(out, relu=True))
    net.finalize()
    outs, ran = _forward(net, batch, dev)
    assert variant in ran, (what, ran)
    _lifted_is_placed(outs[tin], batch)
    conv = PW.PLACEMENTS[placement]["conv"]
    assert tuple(outs[tap].shape[2:]) == (PW.out_size(conv, batch.shape[2]), PW.out_size(conv, batch.shape[3]))
    _check(outs[tap], pairs, "%s (%d, %s, %s)" % (what, variant, precision, placement))


def _w3(cin, cout, transposed=False, k=3, std=0.05):
    return _g(0, "w", (cin, cout, k, k) if transposed else (cout, cin, k, k), std)


# ---- f16c: the compensated patch kernels -------------------------------------------------------------------------------------------------------------------------------
# name: (cin, cout, placement (tests/position_windows.py: canvas, content size, one offset per image), conv kwargs, variant that must run the layer).  Geometries: the smallest
# at which each form is eligible (FORMS of test_hip_f16c_range.py).
F16C = {
    "c16_zero": (256, 256, "zero64_n16", dict(pad=1), 971256),                               # conv3x3_halo_c16.hip, 16 x 64 x 64
    "c16_reflect": (256, 256, "reflect64_n16", dict(pad=1, reflect=True), 971256),
    "c128_zero": (256, 256, "zero64_n8", dict(pad=1), 970128),                               # conv3x3_halo_c.hip, 128 columns, 8 x 64 x 64
    "c128_reflect": (256, 256, "reflect64_n8", dict(pad=1, reflect=True), 970128),
    "c256_ragged": (256, 256, "zero_ragged", dict(pad=1), 970256),                           # 256 columns, 8 x 76 x 92: windows in the partial patches
    "s2_128_256": (128, 256, "zero_s2", dict(stride=2, pad=1), 990256),                      # FORM 2, 8 x 128 x 128
    "s2_64_128": (64, 128, "zero_s2", dict(stride=2, pad=1), 990256),
    "ct_256_128": (256, 128, "zero_t2", dict(stride=2, pad=1, transposed=True), 980256),     # FORM 1, 8 x 64 x 64
    "ct_128_64": (128, 64, "zero_t2", dict(stride=2, pad=1, transposed=True), 980256),
}


@pytest.mark.parametrize("form", list(F16C))
def test_compensated_conv_is_translation_exact(cuda_device, form):
    cin, cout, placement, kw, variant = F16C[form]
    _layer_case(cuda_device, "f16c", placement, cin, _w3(cin, cout, kw.get("transposed", False)), kw, variant, form)


def test_compensated_conv_epilogue_residual_is_translation_exact(cuda_device):
    """the layer of test_halo_c_conv3x3_epilogue_residual (8 x 64 x 64): y = x + BN(conv(pad(x))), BatchNorm folded, the residual t0 added in the
    epilogue.  The layer pads by reflection, so the content keeps one pixel off the canvas border (zero canvas; placement zero64_inner)"""
    c = 256
    bn = (1.0 + _g(0, "g", (c,), 0.2), _g(0, "be", (c,), 0.2), _g(0, "m", (c,), 0.3), 0.5 + _g(0, "v", (c,), 0.1).abs())
    _layer_case(cuda_device, "f16c", "zero64_inner", c, _w3(c, c), dict(pad=1, reflect=True), 970128, "epilogue residual", bias=False, bn=bn, residual=True)


def _stem_case(dev, placement, kw, bn, what):
    """the f16c stem (conv_stem.hip on augmented pixel words, 955000 + taps) on the image itself, as test_stem_c runs it: 4 x 3 x 256 x 256"""
    batch, pairs = PW.place(placement, _content(placement))
    net = HipNet(dev, "f16c")
    bnp = None
    if bn:
        bnp = (synth._uniform(0, "g", (64,), 0.5, 1.5), _g(0, "be", (64,), 0.2), _g(0, "m", (64,), 0.2), synth._uniform(0, "v", (64,), 0.5, 1.5))
    raw = net.conv(net.input(3), _g(0, "w", (64, 3, 7, 7), 0.1), None, bn=bnp, relu=bn, **kw)
    tap = net.output_nchw(raw)
    if not bn:
        net.output_nchw(net.instance_norm(raw, relu=True))          # (test_stem_c's consumer: the statistics epilogue runs; its result is not compared)
    net.finalize()
    outs, ran = _forward(net, batch, dev)
    assert ran and ran[0] // 1000 == 955, (what, ran)
    _check(outs[tap], pairs, "%s (%d, f16c, %s)" % (what, ran[0], placement))


def test_stem_c_reflect_is_translation_exact(cuda_device):
    """7 x 7 reflect stem: the content in both canvas corners against its three-pixel reflect extension in the interior"""
    _stem_case(cuda_device, "reflect7_256", dict(pad=3, reflect=True), False, "stem 7x7 reflect")


def test_stem_c_stride2_is_translation_exact(cuda_device):
    """Conv2d(3, 64, 7, stride 2, zero padding 3) + folded BatchNorm + ReLU: even offsets"""
    _stem_case(cuda_device, "zero_s2k7", dict(stride=2, pad=3), True, "stem 7x7 stride 2")


def test_head7_f32_input_is_translation_exact(cuda_device):
    """conv_head7.hip reading the mode's fp32 tensor (no folded norm), ReflectionPad2d(3) + Conv2d(64, 3, 7), as test_head7_f32_input runs it
    (4 x 128 x 160): three-pixel reflect pairing"""
    _layer_case(cuda_device, "f16c", "reflect7_128x160", 64, _g(0, "w", (3, 64, 7, 7), 0.02), dict(pad=3, reflect=True, out_f32=True, act=0), 920007, "head 7x7")


# ---- f16c: the folded-norm staging modes, reached with the roll family ------------------------------------------------------------------------------------------------
# MODE 1 (norm + ReLU), MODE 2 (norm + residual) and MODE 4 (write-back) are what the InstanceNorm generator runs.  Rolling an image must not change the statistics by one
# bit: the lifted tensor is made of small integers (image values integers in [-4, 4], lift weights in {-1, 0, 1}: |t0| <= 12), so every fp32 partial of sum x and sum x^2
# over 64 x 64 pixels is exact (144 * 4096 < 2^24) in whatever order the conv epilogue records and in_stats_kernel add them.  The normalised values the conv then consumes
# are general fp32 numbers: both halves of the correction product are live.

def _integer_image(seed):
    return torch.randint(-4, 5, (3, 64, 64), generator=torch.Generator().manual_seed(seed)).float()


def _integer_lift(seed, cout):
    return torch.randint(-1, 2, (cout, 3, 1, 1), generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("n,variant", [(16, 971256), (8, 970128)])
@pytest.mark.parametrize("mode", ["norm_relu", "norm_residual_writeback"])
def test_compensated_conv_folded_norm_is_roll_exact(cuda_device, mode, n, variant):
    """norm_relu: conv(instance_norm(t0, relu=True)) -- MODE 1, the conv output compared.  norm_residual_writeback: conv(instance_norm(t0, residual=r)) with the
    normalised tensor tapped -- MODE 2 + 4, the conv output and the written-back tensor compared.  (The norm behind the conv's OWN output is in the graph, as in
    test_halo_c_conv3x3, so that the statistics epilogue runs; it is not compared: its statistics are not exactly summable.)"""
    c = 256
    placement = "roll64_n%d" % n
    image = _integer_image(21)
    batch, pairs = PW.place(placement, image)
    _, flat = PW.place(placement, image, depth=0)
    res = mode == "norm_residual_writeback"
    net = HipNet(cuda_device, "f16c")
    xin = net.input(3)
    t0 = net.conv(xin, _integer_lift(22, c))
    tin = net.output_nchw(t0)
    r = net.conv(xin, _integer_lift(23, c)) if res else -1
    t = net.instance_norm(t0, relu=not res, residual=r)
    out = net.conv(t, _w3(c, c), _g(0, "b", (c,), 0.2), pad=1, reflect=True)
    tap = net.output_nchw(out)
    net.output_nchw(net.instance_norm(out, relu=True))
    twb = net.output_nchw(t) if res else None
    net.finalize()
    outs, ran = _forward(net, batch, cuda_device)
    assert variant in ran, (mode, ran)
    assert net.plan_summary(n, 64, 64)["norms_folded"] >= 1                  # the conv's staging applies the norm: the fold modes are what ran
    lifted = outs[tin].cpu()
    assert torch.equal(lifted, lifted.round()) and float(lifted.abs().max()) <= 12 and PW.compare(lifted, flat).ok          # precondition: exact integers, rolled
    _check(outs[tap], pairs, "%s, conv output (%d, %s)" % (mode, variant, placement))
    if res:
        _check(outs[twb], flat, "%s, written-back tensor (%d, %s)" % (mode, variant, placement))


# ---- the other precisions: a zero-canvas and a reflect case per kernel file that stages a halo (the transposed, stride-2 and 4 x 4 forms pad with zeros only; the heads
# with reflection only) -------------------------------------------------------------------------------------------------------------------------------------------------
# Geometries from the case tables of the tests that pin each kernel (test_hip_layer_bounds.py RB256 / HALO / CT, test_hip_layers.py), on the 8 x 64 x 64 placements.

F16 = {
    "910256_zero": (256, 256, "zero64_n8", dict(pad=1), 910256, False),                              # conv3x3_halo_rb.hip, 256 columns
    "910256_reflect": (256, 256, "reflect64_n8", dict(pad=1, reflect=True), 910256, False),
    "910128_zero": (128, 128, "zero64_n8", dict(pad=1, relu=True), 910128, False),                   # ... four-wave form
    "910128_reflect": (128, 128, "reflect64_n8", dict(pad=1, reflect=True, relu=True), 910128, False),
    "960256_zero": (128, 64, "zero_t2", dict(stride=2, pad=1, transposed=True), 960256, False),      # ... transposed form
    "900064_zero": (64, 64, "zero64_n8", dict(pad=1), 900064, True),                                 # conv3x3_halo.hip (LDS-resident weights): the statistics forms of HALO
    "900128_reflect": (128, 128, "reflect64_n8", dict(pad=1, reflect=True), 900128, True),
}


@pytest.mark.parametrize("form", list(F16))
def test_f16_patch_conv_is_translation_exact(cuda_device, form):
    cin, cout, placement, kw, variant, stats = F16[form]
    _layer_case(cuda_device, "f16", placement, cin, _w3(cin, cout, kw.get("transposed", False)), kw, variant, form, stats=stats)


def test_f16_head7_is_translation_exact(cuda_device):
    """conv_head7.hip's fp16-input form with the tanh (test_generator_head_7x7_tanh): a pointwise activation keeps equal values equal"""
    _layer_case(cuda_device, "f16", "reflect7_128x160", 64, _g(0, "w", (3, 64, 7, 7), 0.03), dict(pad=3, reflect=True, out_f32=True, act=1), 920007, "head 7x7 tanh")


# conv3x3_halo_x3.hip (the exact mode's patch kernel; three fp16 passes per product): FORM 0 (3 x 3), FORM 1 (the transposed conv's phase launches), FORM 2 (stride 2),
# forced below their tile threshold as in test_generator_exact_mode_patch_kernel_forms
F16X3 = {
    "form0_zero": (256, 256, "zero64_n8", dict(pad=1), 930128),
    "form0_reflect": (256, 256, "reflect64_n8", dict(pad=1, reflect=True), 930128),
    "form1_ct_256_128": (256, 128, "zero_t2", dict(stride=2, pad=1, transposed=True), 931128),
    "form1_ct_128_64": (128, 64, "zero_t2", dict(stride=2, pad=1, transposed=True), 931128),        # 64 output channels padded to the 128-column tile
    "form2_s2_128_256": (128, 256, "zero_s2", dict(stride=2, pad=1), 932128),
}


@pytest.mark.parametrize("form", list(F16X3))
def test_f16x3_patch_conv_is_translation_exact(cuda_device, monkeypatch, form):
    monkeypatch.setenv("GDT_CONV_HALO_X3", "2")
    monkeypatch.setenv("GDT_CONV_HALO_X3_FORMS", "2")
    cin, cout, placement, kw, variant = F16X3[form]
    _layer_case(cuda_device, "f16x3", placement, cin, _w3(cin, cout, kw.get("transposed", False)), kw, variant, form)


# conv4x4_halo.hip (PatchGAN discriminator layers: Conv2d(k4, p1), LeakyReLU, zero padding) and conv4x4t_halo.hip (the U-Net's ConvTranspose2d(k4, s2, p1) of a
# concatenation, ReLU on read): LeakyReLU(0) = ReLU(0) = 0 keeps the zero canvas zero.  The case tables of test_hip_discriminator.py / test_hip_unet.py hold maps of a
# few patches; the canvases here are the smallest on which eight placements still cover the patch (placements zero_s2k4, zero_s1k4, zero_t4)
F16_K4 = {
    "906128_s2_64_128": (64, 128, "zero_s2k4", dict(stride=2, pad=1, leaky=0.2), 906128),
    "906256_s2_128_256": (128, 256, "zero_s2k4", dict(stride=2, pad=1, leaky=0.2), 906256),
    "905256_s1_256_512": (256, 512, "zero_s1k4", dict(pad=1, leaky=0.2), 905256),
}


@pytest.mark.parametrize("form", list(F16_K4))
def test_f16_conv4x4_is_translation_exact(cuda_device, form):
    cin, cout, placement, kw, variant = F16_K4[form]
    _layer_case(cuda_device, "f16", placement, cin, _w3(cin, cout, k=4), kw, variant, form)


@pytest.mark.parametrize("cin_a,cin_b", [(64, 64), (128, 0)])
def test_f16_conv4x4_transposed_is_translation_exact(cuda_device, cin_a, cin_b):
    batch, pairs = PW.place("zero_t4", _content("zero_t4"))
    net = HipNet(cuda_device, "f16")
    t = net.input(3)
    a = net.conv(t, _g(0, "wa", (cin_a, 3, 1, 1), 0.7))
    b = net.conv(t, _g(0, "wb", (cin_b, 3, 1, 1), 0.7)) if cin_b else -1
    out = net.conv_transposed4(a, _g(0, "w", (cin_a + cin_b, 64, 4, 4), 0.05), b, relu_a=True, bias=_g(0, "b", (64,), 0.2), relu=True)
    tap = net.output_nchw(out)
    net.finalize()
    outs, ran = _forward(net, batch, cuda_device)
    assert 907064 in ran, ran
    assert tuple(outs[tap].shape[2:]) == (70, 74)
    _check(outs[tap], pairs, "conv4x4t %d + %d (907064, f16, zero_t4)" % (cin_a, cin_b))
