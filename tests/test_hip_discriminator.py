"""The PatchGAN discriminator on the device: the three layer shapes of conv4x4_halo.hip alone against a float64 convolution under a derived bound (patch kernel
and generic path), the whole network against the reference's logits (tests/golden/discriminator.npz) in both precisions, gdt_patch_score / DiscriminatorLoss,
the planner's counter and the rejected configurations, generator -> discriminator on one stream.

Measured on an MI355X, whole net in f16, max|d| / max|ref| over f16_emulated_err (gate: 2), fixture cases 0-4: 1.09, 0.95, 1.38, 0.69, 0.86
(max|d| / max|ref| 9.3e-4, 7.0e-4, 7.7e-4, 6.1e-4, 8.4e-4); f16x3: 0.8e-6 .. 2.0e-6 of the range (gate 1e-5).  Layer test: at most 0.57 of the bound."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gandtr_amd import engine
from gandtr_amd.tools import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "discriminator.npz"))
N_CASES = int(GOLD["n_cases"])
SLOPE = 0.2

# (cin, cout, stride, n, OUTPUT height, OUTPUT width, input height, input width): ragged patches at the right and bottom edges (stride 2: 8 x 16 patches,
# stride 1: 16 x 16), odd output sizes, an odd input size whose last row / column no tap reads, a map smaller than one patch
LAYERS = [(64, 128, 2, 2, 37, 45, 74, 91), (128, 256, 2, 2, 18, 23, 36, 47), (256, 512, 1, 2, 9, 11, 10, 12), (256, 512, 1, 2, 5, 5, 6, 6)]


def _f16(t):
    return t.half().float()


def _layer_reference(a, w, bias, bn, stride, leaky):
    """float64 conv of the fp16-representable input ``a`` with the weights AS PACKED (BatchNorm folded in fp32 like the builder, rounded to fp16), the folded
    shift, the activation; and sum |a| |w| per output"""
    if bn is not None:
        g, be, m, v = (t.numpy().astype(np.float32) for t in bn)
        s = g / np.sqrt(v + np.float32(1e-5))
        shift = be + (bias.numpy().astype(np.float32) - m) * s
        wf = w.numpy().astype(np.float32) * s[:, None, None, None]
    else:
        shift, wf = bias.numpy().astype(np.float32), w.numpy().astype(np.float32)
    wp = torch.from_numpy(wf).half().double()
    pre = F.conv2d(a.double(), wp, torch.from_numpy(shift).double(), stride=stride, padding=1)
    mag = F.conv2d(a.double().abs(), wp.abs(), None, stride=stride, padding=1) + torch.from_numpy(np.abs(shift)).double()[None, :, None, None]
    y = torch.where(pre > 0, pre, pre * float(np.float32(leaky))) if leaky else pre
    return y, mag


@pytest.mark.parametrize("leaky,with_bn", [(0.0, False), (SLOPE, False), (0.0, True), (SLOPE, True)])
@pytest.mark.parametrize("layer", LAYERS, ids=lambda l: "%dto%d_s%d_%dx%d" % (l[0], l[1], l[2], l[4], l[5]))
def test_layer_against_float64(cuda_device, monkeypatch, layer, leaky, with_bn):
    """per output: |got - ref| <= K 2^-24 sum|a||w| + 2^-11 |ref| with K = 16 Cin -- fp32 accumulation of K products (each exact: fp16 x fp16), then the fp16 store.
    Both the patch kernel and (GDT_CONV4X4_HALO=0) the generic implicit GEMM meet it; they need not be bit-equal."""
    cin, cout, stride, n, oh, ow, ih, iw = layer
    monkeypatch.delenv("GDT_CONV4X4_HALO", raising=False)
    net = engine.HipNet(cuda_device, "f16")
    t = net.input(3)
    a = net.conv(t, synth._normal(1, "w0", (cin, 3, 1, 1), 0.7), synth._normal(1, "b0", (cin,), 0.2))
    tap_in = net.output_nchw(a)
    w = _f16(synth._normal(2, "w4", (cout, cin, 4, 4), (2.0 / (cin * 16)) ** 0.5))
    b = synth._normal(2, "b4", (cout,), 0.1)
    bn = None
    if with_bn:
        sd = {}
        synth._bn(sd, 3, "bn", cout)
        bn = (sd["bn.weight"], sd["bn.bias"], sd["bn.running_mean"], sd["bn.running_var"])
    tap = net.output_nchw(net.conv(a, w, b, bn=bn, stride=stride, pad=1, leaky=leaky))
    net.finalize()
    assert net.output_shapes(n, ih, iw)[tap] == (n, cout, oh, ow)
    assert net.conv4x4_launches(n, ih, iw) == 1
    x = synth.synth_input(4, (n, 3, ih, iw)).to(cuda_device)
    net.set_profiling(True)
    outs = net.forward(x)
    torch.cuda.synchronize()
    variants = [v for k, v, ms, fl in net.profile() if k == 1]
    assert variants[-1] == (905256 if stride == 1 else (906256 if cout % 256 == 0 else 906128)), variants       # conv4x4_halo.hip: stride 1, stride 2 in 256 / 128 columns
    net.set_profiling(False)
    assert torch.equal(outs[tap], net.forward(x)[tap])
    xin, got = outs[tap_in].cpu(), outs[tap].cpu().double()
    monkeypatch.setenv("GDT_CONV4X4_HALO", "0")
    assert net.conv4x4_launches(n, ih, iw) == 0
    generic = net.forward(x)[tap].cpu().double()
    monkeypatch.delenv("GDT_CONV4X4_HALO")
    assert torch.equal(_f16(xin), xin)
    ref, mag = _layer_reference(xin, w, b, bn, stride, leaky)
    bound = 16 * cin * 2.0 ** -24 * mag + 2.0 ** -11 * ref.abs()
    for name, y in (("conv4x4_halo", got), ("generic", generic)):
        excess = float(((y - ref).abs() / bound).max())
        print("%s %s leaky %s bn %s: max |d| / bound = %.3f, max|d| %.3e" % (name, layer, leaky, with_bn, excess, float((y - ref).abs().max())))
        assert excess <= 1.0, name


def _case(i, dev, precision):
    from gandtr_amd.components.model.network import p2p_networks
    p = "c%d_" % i
    ndf, n_layers, wseed, xseed = (int(v) for v in GOLD[p + "cfg"])
    norm = str(GOLD[p + "norm"])
    model = p2p_networks.NLayerDiscriminator(3, ndf=ndf, n_layers=n_layers, norm_layer=norm).eval()
    model.load_state_dict(synth.discriminator_state(wseed, norm, ndf=ndf, n_layers=n_layers, gain=float(GOLD["gain"])))
    model.hip_precision = precision
    x = synth.synth_input(xseed, tuple(int(v) for v in GOLD[p + "shape"]), 1.0)
    return model.to(dev), x.to(dev), torch.from_numpy(GOLD[p + "logits"]), float(GOLD[p + "f16_emulated_err"])


@pytest.mark.parametrize("i", range(N_CASES))
def test_whole_net_f16(cuda_device, i):
    """max|d| / max|ref| <= 2 x f16_emulated_err: the emulation rounds weights and conv inputs to fp16; the factor 2 covers the fp16 storage of the conv outputs
    that feed the InstanceNorm and the accumulation order, which it does not model"""
    model, x, ref, emu = _case(i, cuda_device, "f16")
    with torch.no_grad():
        got = model(x).cpu()
    assert got.shape == ref.shape
    rel = float((got - ref).abs().max() / ref.abs().max())
    print("case %d f16: max|d| / max|ref| = %.3e = %.2f x f16_emulated_err (%.3e)" % (i, rel, rel / emu, emu))
    assert rel <= 2 * emu


@pytest.mark.parametrize("i", range(N_CASES))
def test_whole_net_f16x3(cuda_device, i):
    model, x, ref, _ = _case(i, cuda_device, "f16x3")
    with torch.no_grad():
        got = model(x).cpu()
    rel = float((got - ref).abs().max() / ref.abs().max())
    print("case %d f16x3: max|d| / max|ref| = %.3e" % (i, rel))
    assert rel <= 1e-5


def _terms64(v, t, kind):
    if kind == "mse":
        return (v - t) ** 2
    return v.clamp(min=0) - v * t + torch.log1p(torch.exp(-v.abs()))


@pytest.mark.parametrize("kind", ["mse", "bce_with_logits"])
@pytest.mark.parametrize("shape", [(5, 1, 7, 9), (3, 1, 30, 30), (2, 1, 1, 1)])
def test_patch_scores(cuda_device, kind, shape):
    """per image within h w 2^-24 mean|term| of float64, bit-identical over two runs, equal to the CPU DiscriminatorLoss path within that bound"""
    from gandtr_amd.components.optim.criterion import adversarial
    y = synth._normal(7, "logits", shape, 3.0)
    yd = y.to(cuda_device)
    s1, s2 = adversarial.patch_scores(yd, kind), adversarial.patch_scores(yd, kind)
    for a, b in zip(s1, s2):
        assert a.is_cuda and a.dtype == torch.float64 and torch.equal(a, b)
    v = y.double().reshape(shape[0], -1)
    hw = v.shape[1]
    wants = (v, _terms64(v, 0.0, kind), _terms64(v, 1.0, kind))
    for got, terms in zip(s1[:3], wants):
        bound = hw * 2.0 ** -24 * terms.abs().mean(dim=1)
        err = (got.cpu() - terms.mean(dim=1)).abs()
        print("%s %s: max err / bound %.3e" % (kind, shape, float((err / bound).max())))
        assert bool((err <= bound).all())
    for k, terms in enumerate(wants):
        assert abs(float(s1.total[k].cpu()) - float(terms.mean())) <= hw * 2.0 ** -24 * float(terms.abs().mean())
    crit = adversarial.DiscriminatorLoss(criterion={"loss": kind})
    for real in (True, False):
        dev_loss, cpu_loss = crit(yd, real, cuda_device), crit(y, real, "cpu")
        assert dev_loss.total.is_cuda and dev_loss.total.dtype == torch.float32
        terms = wants[1 + int(not real)]                        # a real target is 0, a fake target is 1
        assert abs(float(dev_loss.total.cpu()) - float(cpu_loss.total)) <= hw * 2.0 ** -24 * float(terms.abs().mean())
    y2 = synth._normal(8, "logits2", (shape[0], 1, 4, 5), 2.0)
    both, both_cpu = crit([yd, y2.to(cuda_device)], True, cuda_device), crit([y, y2], True, "cpu")
    assert set(both.partial) == {"layer1", "layer0"}
    assert float(both.total.cpu()) == pytest.approx(float(both_cpu.total), rel=1e-6)
    assert float(both.total.cpu()) == pytest.approx(float(both.partial["layer1"].cpu()) + float(both.partial["layer0"].cpu()), rel=1e-6)


def test_planner_counter_and_rejections(cuda_device, monkeypatch):
    monkeypatch.delenv("GDT_CONV4X4_HALO", raising=False)
    model, x, ref, emu = _case(0, cuda_device, "f16")
    net = engine.build_discriminator({k: v.cpu() for k, v in model.state_dict().items()}, cuda_device)
    n, _, h, w = x.shape
    assert net.conv4x4_launches(n, h, w) == 3 and net.conv4x4_launches(64, 256, 256) == 3
    on = net.forward(x)[net.out_slot].cpu()
    monkeypatch.setenv("GDT_CONV4X4_HALO", "0")
    assert net.conv4x4_launches(n, h, w) == 0
    off = net.forward(x)[net.out_slot].cpu()                   # the same net wholly on the generic path
    monkeypatch.delenv("GDT_CONV4X4_HALO")
    for y in (on, off):
        assert float((y - ref).abs().max() / ref.abs().max()) <= 2 * emu
    model.hip_precision = "f16c"
    with pytest.raises(NotImplementedError):
        model(x)
    model.hip_precision = "f16ch"
    with pytest.raises(NotImplementedError):
        model(x)
    bn_model, xb, _, _ = _case(1, cuda_device, "f16")
    bn_model.train()
    with pytest.raises(NotImplementedError):
        with torch.no_grad():
            bn_model(xb)


def test_generator_into_discriminator_on_one_stream(cuda_device):
    """discriminator(generator(x)) without a host copy in between, on one (side) stream, equals the two calls made separately bit for bit"""
    from gandtr_amd.components.model.network import p2p_networks
    gen = p2p_networks.ResnetGenerator(3, 3, ngf=16, norm_layer="instance", n_blocks=2).eval()
    gen.load_state_dict(synth.generator_state(0, "instance", ngf=16, n_blocks=2))
    disc = p2p_networks.NLayerDiscriminator(3, norm_layer="instance").eval()
    disc.load_state_dict(synth.discriminator_state(0, "instance", gain=0.2))
    gen, disc = gen.to(cuda_device), disc.to(cuda_device)
    x = synth.synth_input(9, (2, 3, 64, 64), 1.0).to(cuda_device)
    side = torch.cuda.Stream(cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.no_grad(), torch.cuda.stream(side):
        fake = gen(x)
        chained = disc(fake)
        assert fake.is_cuda and chained.is_cuda
    side.synchronize()
    with torch.no_grad():
        fake2 = gen(x)
        torch.cuda.synchronize(cuda_device)
        separate = disc(fake2.clone())
    torch.cuda.synchronize(cuda_device)
    assert tuple(chained.shape) == (2, 1, 6, 6)
    assert torch.equal(fake, fake2) and torch.equal(chained, separate)
    assert bool(torch.isfinite(chained).all())
