"""``outconv_dynint_unet`` on the device: the resize op alone against a float64 evaluation of torch's coordinate formula under a derived per-element bound, the
LeakyReLU Conv(k4, s2, p1) at odd sizes on both of its routes under the bound of tests/conv_bound.py, every dynint net of tests/golden/orig_unet.npz against the
reference's map in both precisions, the module's forward against the builder's graph, a size no other net of the family accepts, the rejected
configurations.

Measured figures (MI355X) are in the docstrings of the tests."""
import json
import os

import numpy as np
import pytest
import torch

import conv_bound as CB
from gandtr_amd import engine
from gandtr_amd.components.model.network import unet
from gandtr_amd.tools import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "orig_unet.npz"))
CASES = [i for i in range(int(GOLD["n_cases"])) if str(GOLD["c%d_label" % i]) == "outconv_dynint_unet"]
OUT_CHANNELS = int(GOLD["out_channels"])

# (H, W) of the large map: the small one is its Conv(k4, s2, p1), floor(H / 2) x floor(W / 2): 5x7 -> 11x15, 1x1 -> 2x3, 8x8 -> 16x16, 18x25 -> 37x50
RESIZES = [(11, 15), (2, 3), (16, 16), (37, 50)]
CHANNELS = 64


def _resize_net(dev, mode, precision="f16"):
    """input -> 1x1 conv (the tensor whose size is the target) -> Conv(k4, s2, p1) (the small map, tapped) -> resize to the target -> tap; and the small map
    resized to its own size"""
    net = engine.HipNet(dev, precision)
    like = net.conv(net.input(3), synth._normal(1, "wa", (16, 3, 1, 1), 0.7), synth._normal(1, "ba", (16,), 0.2))
    small = net.conv(like, synth._normal(1, "wb", (CHANNELS, 16, 4, 4), 0.1), synth._normal(1, "bb", (CHANNELS,), 0.2), stride=2, pad=1)
    tap = net.output_nchw(small)
    out = net.output_nchw(net.resize(small, like, mode))
    same = net.output_nchw(net.resize(small, small, mode))
    net.finalize()
    return net, tap, out, same


def _axis(n_in, n_out):
    """torch's source coordinates of F.interpolate(size=.., mode="bilinear", align_corners=False) along one axis, in float64: (i0, i1, lambda)"""
    scale = np.float64(n_in) / np.float64(n_out)
    src = np.maximum(scale * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    return i0, i0 + (i0 < n_in - 1), src - i0


@pytest.mark.parametrize("size", RESIZES, ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("precision", ["f16", "f16x3"])
def test_bilinear_resize_against_float64(cuda_device, size, precision):
    """out = (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11) evaluated in float64 on the tapped tensor.

    Bound, with u = 2^-24 and m = max |tap| over the four taps of an output.  Coordinates: the kernel takes lambda as the exact remainder over 2 out, rounded
    once, so each axis has |d lambda| <= u / 2 and |d (1 - lambda)| <= u (its own rounding on top): at most one ulp of lambda per axis.  The four weights
    w_y w_x then move by sum (w_y |d w_x| + w_x |d w_y|) = (sum |d w_x|) + (sum |d w_y|) <= 3 u, times m.  Arithmetic: every tap goes through three fp32
    operations (product, sum, product) and the final sum, each rounding u / 2 of a value bounded by m, the weights summing to 1: <= 2 u m.  Together
    5 u m + second order <= e = 8 u m = 8 * 2^-24 max|taps|.  Then ONE store in the tensor's type: fp16 adds 2^-11 (|ref| + e) + 2^-25 (conv_bound.py); the
    fp32 store of f16x3 adds u (|ref| + e) instead.  MEASURED on an MI355X, max |d| / bound in the order of RESIZES: f16 0.991, 0.000, 0.996, 0.998 (the half
    ulp of the fp16 store; 1x1 -> 2x3 copies its one pixel), f16x3 0.306, 0.171, 0.222, 0.296."""
    H, W = size
    net, tap, out, same = _resize_net(cuda_device, "bilinear", precision)
    x = synth.synth_input(3, (2, 3, H, W)).to(cuda_device)
    outs = net.forward(x)
    v = outs[tap].cpu().double()
    h, w = v.shape[2:]
    assert (h, w) == (H // 2, W // 2) and tuple(outs[out].shape) == (2, CHANNELS, H, W)
    y0, y1, ly = _axis(h, H)
    x0, x1, lx = _axis(w, W)
    ly_, lx_ = torch.from_numpy(ly)[None, None, :, None], torch.from_numpy(lx)[None, None, None, :]
    g = lambda yy, xx: v[:, :, yy][:, :, :, xx]
    v00, v01, v10, v11 = g(y0, x0), g(y0, x1), g(y1, x0), g(y1, x1)
    ref = (1 - ly_) * ((1 - lx_) * v00 + lx_ * v01) + ly_ * ((1 - lx_) * v10 + lx_ * v11)
    m = torch.stack([v00.abs(), v01.abs(), v10.abs(), v11.abs()]).max(0).values
    e = 8 * CB.U32 * m
    bound = e + (CB.U16 * (ref.abs() + e) + CB.SUB16 if precision == "f16" else CB.U32 * (ref.abs() + e))
    got = outs[out].cpu().double()
    q = float(((got - ref).abs() / bound).max())
    print("bilinear %dx%d -> %dx%d %s: max |d| / bound = %.3f" % (h, w, H, W, precision, q))
    assert q <= 1.0
    assert torch.equal(outs[same], outs[tap])                         # equal sizes: a bit-exact copy
    assert torch.equal(net.forward(x)[out], outs[out])                # bit-identical run to run


@pytest.mark.parametrize("size", RESIZES, ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("precision", ["f16", "f16x3"])
def test_nearest_resize_is_an_index_gather(cuda_device, size, precision):
    """nearest: i = min(floor(dst * scale), in - 1) with scale = in / out in fp32, as torch computes it: bit-exact against the gather and against torch"""
    H, W = size
    net, tap, out, same = _resize_net(cuda_device, "nearest", precision)
    x = synth.synth_input(3, (2, 3, H, W)).to(cuda_device)
    outs = net.forward(x)
    v = outs[tap].cpu()
    h, w = v.shape[2:]
    idx = lambda n_in, n_out: np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * (np.float32(n_in) / np.float32(n_out))).astype(np.int64), n_in - 1)
    ref = v[:, :, idx(h, H)][:, :, :, idx(w, W)]
    assert torch.equal(outs[out].cpu(), ref)
    assert torch.equal(outs[out].cpu(), torch.nn.functional.interpolate(v, size=(H, W), mode="nearest"))
    assert torch.equal(outs[same], outs[tap])


# ------------------------------------------------------------------------------------------------ Conv(k4, s2, p1) + LeakyReLU at odd sizes
@pytest.mark.parametrize("geometry", [(2, 37, 25), (2, 5, 7)], ids=lambda v: "_".join(str(e) for e in v))
def test_leaky_conv4x4_stride2_at_odd_sizes(cuda_device, monkeypatch, geometry):
    """the down convs of the net meet odd maps at every level: 64 -> 128, Conv(k4, s2, p1) + LeakyReLU(0.2), output floor(H / 2) x floor(W / 2), on
    conv4x4_halo.hip and on the generic route (GDT_CONV4X4_HALO=0) under the derived bound of conv_bound.layer.  MEASURED on an MI355X: max |d| / bound 0.521 (2 x 37 x 25) and
    0.463 (2 x 5 x 7), the same on both routes: conv4x4_halo.hip is correct at odd sizes and keeps them."""
    n, h, w_ = geometry
    net = engine.HipNet(cuda_device, "f16")
    a = net.conv(net.input(3), synth._normal(1, "wa", (64, 3, 1, 1), 0.7), synth._normal(1, "ba", (64,), 0.2))
    tap = net.output_nchw(a)
    w = CB.f16(synth._normal(2, "wd", (128, 64, 4, 4), (2.0 / (64 * 16)) ** 0.5))
    bias = synth._normal(2, "bd", (128,), 0.1)
    out = net.output_nchw(net.conv(a, w, bias, stride=2, pad=1, leaky=0.2))
    net.finalize()
    assert net.output_shapes(n, h, w_)[out] == (n, 128, h // 2, w_ // 2)
    x = synth.synth_input(4, (n, 3, h, w_)).to(cuda_device)
    wp, shift = CB.fold(w, bias)
    monkeypatch.delenv("GDT_CONV4X4_HALO", raising=False)
    assert net.conv4x4_launches(n, h, w_) == 1
    for name, knob in (("conv4x4_halo", None), ("generic", "0")):
        if knob is not None:
            monkeypatch.setenv("GDT_CONV4X4_HALO", knob)
            assert net.conv4x4_launches(n, h, w_) == 0
        outs = net.forward(x)
        CB.assert_layer(outs[out].cpu(), outs[tap].cpu(), wp, shift, "%s leaky k4 s2 %s" % (name, geometry), stride=2, pad=1, act="leaky", leaky=0.2)
        assert torch.equal(net.forward(x)[out], outs[out])
    monkeypatch.delenv("GDT_CONV4X4_HALO")


# ------------------------------------------------------------------------------------------------ the whole nets
def _case(i, dev, precision):
    """(module on the device, input, the reference's output, f16_emulated_err)"""
    p = "c%d_" % i
    cfg = json.loads(str(GOLD[p + "cfg"]))
    shape = tuple(int(v) for v in GOLD[p + "shape"])
    wseed, xseed = (int(v) for v in GOLD[p + "seeds"])
    model = unet.CLASSES["outconv_dynint_unet"](shape[1], OUT_CHANNELS, **cfg).eval()
    model.load_state_dict(synth.dynint_unet_state(wseed, in_channels=shape[1], out_channels=OUT_CHANNELS, **{k: v for k, v in cfg.items() if k != "upsample"}), strict=True)
    model.hip_precision = precision
    return model.to(dev), synth.synth_input(xseed, shape, 1.0).to(dev), torch.from_numpy(GOLD[p + "out"]), float(GOLD[p + "f16_emulated_err"])


def _net(model, dev, precision):
    return engine.build_dynint_unet({k: v.cpu() for k, v in model.state_dict().items()}, dev, model._cfg, precision=precision)


def _rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("i", CASES)
def test_whole_net_f16(cuda_device, i):
    """max|d| / max|ref| <= 2 x f16_emulated_err, the family's gate; bit-identical run to run; the module's forward equals the builder's graph bit for bit.
    MEASURED on an MI355X, max|d| / max|ref| over f16_emulated_err, cases 3-6: 1.20, 1.63, 1.05, 0.74 (max|d| / max|ref| 5.5e-4 .. 8.9e-4)."""
    model, x, ref, emu = _case(i, cuda_device, "f16")
    net = _net(model, cuda_device, "f16")
    got = net.forward(x)[net.out_slot].cpu()
    assert got.shape == ref.shape
    assert torch.equal(got, net.forward(x)[net.out_slot].cpu())
    with torch.no_grad():
        y = model(x)
    assert y.is_cuda and y.dtype == torch.float32 and torch.equal(y.cpu(), got)
    rel = _rel(got, ref)
    print("case %d outconv_dynint_unet f16: max|d| / max|ref| = %.3e = %.2f x f16_emulated_err (%.3e)" % (i, rel, rel / emu, emu))
    assert rel <= 2 * emu


@pytest.mark.parametrize("i", CASES)
def test_whole_net_f16x3(cuda_device, i):
    """1e-5 of max|ref|.  MEASURED on an MI355X, cases 3-6: 8.5e-7, 1.4e-6, 6.5e-7, 4.5e-7"""
    model, x, ref, _ = _case(i, cuda_device, "f16x3")
    net = _net(model, cuda_device, "f16x3")
    got = net.forward(x)[net.out_slot].cpu()
    rel = _rel(got, ref)
    print("case %d outconv_dynint_unet f16x3: max|d| / max|ref| = %.3e" % (i, rel))
    assert rel <= 1e-5


def test_a_size_no_other_family_member_accepts(cuda_device):
    """(1, 3, 45, 67): odd and prime-ish, divisible by nothing the other nets need; against the module's own CPU forward (fp32 torch) under the f16 gate of the
    nearest fixture case (same depth), and in f16x3 within 1e-5.  MEASURED on an MI355X: f16 1.00 x f16_emulated_err, f16x3 9.6e-7"""
    i = CASES[0]
    model, _, _, emu = _case(i, cuda_device, "f16")
    x = synth.synth_input(77, (1, 3, 45, 67), 1.0)
    import copy
    with torch.no_grad():
        ref = copy.deepcopy(model).cpu()(x)
        y = model(x.to(cuda_device)).cpu()
        model.hip_precision = "f16x3"
        y3 = model(x.to(cuda_device)).cpu()
    assert y.shape == ref.shape == (1, OUT_CHANNELS, 45, 67)
    print("dynint 45x67: f16 %.2f x f16_emulated_err, f16x3 %.3e" % (_rel(y, ref) / emu, _rel(y3, ref)))
    assert _rel(y, ref) <= 2 * emu and _rel(y3, ref) <= 1e-5
    for label in ("p2p_unet", "outconv_unet", "aligned_p2p_unet"):
        other = unet.CLASSES[label](3, 3, nested_levels=2).eval().to(cuda_device)
        with torch.no_grad(), pytest.raises(ValueError, match="reflectpad_divisible"):
            other(x.to(cuda_device))


def test_rejections(cuda_device):
    model, x, _, _ = _case(CASES[1], cuda_device, "f16")              # nested_levels 3, BatchNorm
    with torch.no_grad(), pytest.raises(ValueError, match="at least 16"):
        model(synth.synth_input(1, (1, 3, 15, 40), 1.0).to(cuda_device))
    net = _net(model, cuda_device, "f16")
    with pytest.raises(ValueError, match="empty"):                    # ... and the graph itself refuses it
        net.forward(synth.synth_input(1, (1, 3, 15, 40), 1.0).to(cuda_device))
    for prec in ("f16c", "f16ch"):
        model.hip_precision = prec
        with torch.no_grad(), pytest.raises(NotImplementedError):
            model(x)
    model.hip_precision = "f16"
    model.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="inference-only"):
        model(x)
    bicubic = unet.OutconvP2pUNetDynamicInterpolate(3, 3, nested_levels=1, upsample="bicubic").eval().to(cuda_device)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="bicubic"):
        bicubic(torch.zeros(1, 3, 8, 8, device=cuda_device))
    opts = unet.OutconvP2pUNetDynamicInterpolate(3, 3, nested_levels=1, upconv_opts={"kernel_size": 1, "padding": 0}).eval().to(cuda_device)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="upconv_opts"):
        opts(torch.zeros(1, 3, 8, 8, device=cuda_device))
