"""ResnetGenerator with CUT's anti-aliased sampling (no_antialias=False / no_antialias_up=False) without a GPU: the host mirror against the reference's fixtures
(tests/golden/make_antialias_golden.py), state dicts, the layout helpers, and the planner's decisions about the blur-resample ops (host logic: no device call)."""
import os
import subprocess
import sys

import pytest
import torch

import blur_ref as br
from gandtr_amd import engine
from gandtr_amd.components.model import network as M
from gandtr_amd.components.model.network import p2p_networks
from gandtr_amd.tools import synth
from test_host_mirror import close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"        # only recorded; no device call happens before finalize()
FLAGS = [(True, True), (False, True), (True, False), (False, False)]        # (no_antialias, no_antialias_up)


def _gen(norm, no_antialias, no_antialias_up, ngf=8, n_blocks=2):
    gen = M.initialize_model({"architecture": "official_resnet_generator", "input_nc": 3, "output_nc": 3, "ngf": ngf, "n_blocks": n_blocks, "norm_layer": norm,
                              "no_antialias": no_antialias, "no_antialias_up": no_antialias_up}).eval()
    gen.load_state_dict(synth.generator_state(0, norm, ngf=ngf, n_blocks=n_blocks, no_antialias=no_antialias, no_antialias_up=no_antialias_up), strict=True)
    return gen


def _check_taps(gen, x, layers, golden):
    """every stored tap and the output of the mirror on the CPU, within test_host_mirror.py's tolerance; the two padded tensors from their definition"""
    assert len(gen.model) == layers
    with torch.no_grad():
        out, feats = gen(x, layers=list(range(layers)))
    close(out, golden[layers - 1])
    for i, f in enumerate(feats):
        if i in golden:
            close(f[:golden[i].shape[0]], golden[i])
    assert torch.equal(feats[0], torch.nn.functional.pad(x, (3, 3, 3, 3), mode="reflect"))
    assert torch.equal(feats[layers - 3], torch.nn.functional.pad(feats[layers - 4], (3, 3, 3, 3), mode="reflect"))
    return feats


@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_mirror_against_the_reference_fixture(norm):
    layers, golden = br.golden_taps("gen_tiny_aa_" + norm)
    assert layers == 25 and sorted(golden) == [i for i in range(25) if i not in (0, 22)]
    feats = _check_taps(_gen(norm, False, False), synth.synth_input(1, (2, 3, 32, 32), 1.0), layers, golden)
    assert [tuple(feats[i].shape[1:]) for i in (6, 7, 10, 11, 14, 18)] == [(16, 32, 32), (16, 16, 16), (32, 16, 16), (32, 8, 8), (32, 16, 16), (16, 32, 32)]


@pytest.mark.parametrize("tag", ["down", "up", "odd"])
def test_mirror_mixed_flags_and_odd_size(tag):
    """one flag at a time on the 32 x 32 input; both flags off on 1 x 3 x 21 x 18, whose maps go 21 x 18 -> 11 x 9 -> 6 x 5 -> 12 x 10 -> 24 x 20"""
    layers, golden = br.golden_taps("gen_tiny_aa_cases", tag + "_")
    flags = {"down": (False, True), "up": (True, False), "odd": (False, False)}[tag]
    x = synth.synth_input(1, (1, 3, 21, 18), 1.0) if tag == "odd" else synth.synth_input(1, (2, 3, 32, 32), 1.0)
    feats = _check_taps(_gen("instance", *flags), x, layers, golden)
    if tag == "odd":
        assert [tuple(feats[i].shape[2:]) for i in (6, 7, 11, 14, 18, 24)] == [(21, 18), (11, 9), (6, 5), (12, 10), (24, 20), (24, 20)]


def test_sampling_layers_from_their_definitions():
    """Downsample(C) = ReflectionPad2d(1) + depthwise 3 x 3 at stride 2 with outer([1, 2, 1], [1, 2, 1]) / 16, ceil(H / 2) x ceil(W / 2), refusing a 1-pixel axis like
    the reference; Upsample(C) = bilinear x 2 (align_corners=False), defined from 1 x 1; the ``filt`` buffers have the reference's shapes and dyadic values"""
    d, u = p2p_networks.Downsample(4), p2p_networks.Upsample(4)
    assert tuple(d.filt.shape) == (4, 1, 3, 3) and tuple(u.filt.shape) == (4, 1, 4, 4)
    assert torch.equal(d.filt[2, 0] * 16, torch.tensor([[1., 2., 1.], [2., 4., 2.], [1., 2., 1.]]))
    assert torch.equal(u.filt[1, 0] * 16, torch.tensor([1., 3., 3., 1.])[:, None] * torch.tensor([1., 3., 3., 1.])[None, :])
    for h, w in [(5, 7), (16, 16), (2, 3), (2, 2)]:
        x = synth.synth_input(3, (2, 4, h, w)).double()
        assert tuple(d.double()(x).shape) == (2, 4, (h + 1) // 2, (w + 1) // 2)
        assert float((d(x) - br.blur(x, False)).abs().max()) < 1e-14
    for h, w in [(5, 7), (16, 16), (2, 3), (1, 4), (3, 1), (1, 1)]:
        x = synth.synth_input(3, (2, 4, h, w)).double()
        ref = torch.nn.functional.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        assert float((u.double()(x) - ref).abs().max()) < 1e-14 and float((br.blur(x, True) - ref).abs().max()) < 1e-14
    with pytest.raises(RuntimeError):
        p2p_networks.Downsample(4)(torch.zeros(1, 4, 1, 5))


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "aa%d_up%d" % (not f[0], not f[1]))
@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_state_dicts_layout_and_tap_channels(norm, flags):
    """synth's state dict loads strictly into the mirror and the mirror's own into a second one; generator_layout / generator_antialias read the layout from the
    ``filt`` keys; generator_tap_channels matches the channels of every tap of a forward"""
    no_aa, no_aa_up = flags
    sd = synth.generator_state(0, norm, ngf=8, n_blocks=3, in_nc=2, out_nc=5, no_antialias=no_aa, no_antialias_up=no_aa_up)
    gen = p2p_networks.ResnetGenerator(2, 5, ngf=8, norm_layer=norm, n_blocks=3, no_antialias=no_aa, no_antialias_up=no_aa_up).eval()
    gen.load_state_dict(sd, strict=True)
    twin = p2p_networks.ResnetGenerator(2, 5, ngf=8, norm_layer=norm, n_blocks=3, no_antialias=no_aa, no_antialias_up=no_aa_up)
    twin.load_state_dict(gen.state_dict(), strict=True)
    assert set(gen.state_dict()) == set(sd)
    filt = sorted(k for k in sd if k.endswith(".filt"))
    assert filt == sorted((["model.7.filt", "model.11.filt"] if not no_aa else []) +
                          (["model.%d.filt" % i for i in ((15, 19) if not no_aa else (13, 17))] if not no_aa_up else []))
    for k in filt:
        assert torch.equal(sd[k], gen.state_dict()[k]) and sd[k].shape[2] == (3 if k in ("model.7.filt", "model.11.filt") else 4)
    assert engine.generator_antialias(sd) == flags
    assert engine.generator_layout(sd) == (norm, 8, 3, 2, 5)
    layers = len(gen.model)
    assert layers == 19 + 3 + 2 * (not no_aa) + 2 * (not no_aa_up)
    taps = [i for i in range(layers) if i not in (0, layers - 3)]
    with torch.no_grad():
        feats = gen(synth.synth_input(2, (1, 2, 16, 12), 1.0), layers=taps, encode_only=True)
    assert p2p_networks.generator_tap_channels(taps, ngf=8, n_blocks=3, input_nc=2, output_nc=5, no_antialias=no_aa, no_antialias_up=no_aa_up) == \
        [f.shape[1] for f in feats]
    with pytest.raises(NotImplementedError):
        p2p_networks.generator_tap_channels([layers - 3], ngf=8, n_blocks=3, no_antialias=no_aa, no_antialias_up=no_aa_up)
    with pytest.raises(ValueError):
        p2p_networks.generator_tap_channels([layers], ngf=8, n_blocks=3, no_antialias=no_aa, no_antialias_up=no_aa_up)


def test_default_flags_give_the_modules_and_keys_of_before():
    """no flag: the hub configuration -- stride-2 convs and ConvTranspose2d, no ``filt`` key, the tap channels and the state dict of the two-argument calls"""
    gen = p2p_networks.ResnetGenerator(3, 3, ngf=8, norm_layer="instance", n_blocks=2)
    kinds = [type(m).__name__ for m in gen.model]
    assert kinds == ["ReflectionPad2d", "Conv2d", "InstanceNorm2d", "ReLU"] + ["Conv2d", "InstanceNorm2d", "ReLU"] * 2 + ["ResnetBlock"] * 2 + \
        ["ConvTranspose2d", "InstanceNorm2d", "ReLU"] * 2 + ["ReflectionPad2d", "Conv2d", "Tanh"]
    assert gen.model[4].stride == (2, 2) and not any(k.endswith(".filt") for k in gen.state_dict())
    a, b = synth.generator_state(0, "batch", ngf=8, n_blocks=2), synth.generator_state(0, "batch", ngf=8, n_blocks=2, no_antialias=True, no_antialias_up=True)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert a["model.12.weight"].shape == (32, 16, 3, 3)          # ConvTranspose2d: [cin, cout, k, k]
    assert p2p_networks.generator_tap_channels([2, 5, 8], ngf=16, n_blocks=2) == [16, 32, 64]
    assert engine.generator_antialias(a) == (True, True) and engine.generator_layout(a) == ("batch", 8, 2, 3, 3)
    aa = p2p_networks.ResnetGenerator(3, 3, ngf=8, norm_layer="instance", n_blocks=2, no_antialias=False, no_antialias_up=False)
    kinds = [type(m).__name__ for m in aa.model]
    assert kinds[4:12] == ["Conv2d", "InstanceNorm2d", "ReLU", "Downsample"] * 2 and kinds[14:22] == ["Upsample", "Conv2d", "InstanceNorm2d", "ReLU"] * 2
    assert aa.model[4].stride == (1, 1) and aa.model[15].stride == (1, 1)


def test_the_discriminator_still_refuses():
    with pytest.raises(NotImplementedError):
        p2p_networks.NLayerDiscriminator(3, no_antialias=False)


# ------------------------------------------------------------------------------------------------ the planner (host logic, no device)
def _full(norm="instance", precision="f16c", **kw):
    return engine.build_generator(synth.generator_state(0, norm, no_antialias=False, no_antialias_up=False), DEV, precision=precision, finalize=False, **kw)


@pytest.mark.parametrize("precision", ["f16c", "f16", "f16x3"])
def test_planner_folds_the_untapped_norms_into_the_blur_ops(precision, monkeypatch):
    """the full-width net at (64, 256, 256): four blur launches; the norms in front of both Downsamples and of the second Upsample are folded (the first Upsample
    reads the last block's residual norm: not folded).  With the taps [4, 7, 10, 14] the norm in front of index 7 stays folded (tap 4 is the raw conv, tap 7 the
    op's output) and the one in front of index 11 is tapped (10) and keeps its apply pass.  The encoder-only graph ends at tap 14."""
    monkeypatch.delenv("GDT_NORM_FUSION", raising=False)
    net = _full(precision=precision)
    assert net.blur_summary(64, 256, 256) == {"launches": 4, "folded": 3}
    plain = engine.build_generator(synth.generator_state(0, "instance"), DEV, precision=precision, finalize=False)
    # every norm that was folded in the hub net is folded here; the two stride-1 down convs and the Upsamples' convs take their norms like the hub's layers do
    assert net.plan_summary(64, 256, 256)["norms_folded"] >= 3 and plain.blur_summary(64, 256, 256) == {"launches": 0, "folded": 0}
    tapped = _full(precision=precision, taps=(4, 7, 10, 14))
    assert tapped.blur_summary(64, 256, 256) == {"launches": 4, "folded": 2}
    enc = _full(precision=precision, taps=(4, 7, 10, 14), stop_after_taps=True)
    assert enc.blur_summary(64, 256, 256) == {"launches": 2, "folded": 1}
    assert enc.output_shapes(2, 64, 64) == [(2, 128, 64, 64), (2, 128, 32, 32), (2, 256, 32, 32), (2, 256, 16, 16)]
    assert net.output_shapes(1, 21, 18) == [(1, 3, 24, 20)]


def test_planner_batchnorm_net_folds_nothing():
    """BatchNorm is folded into the convs as before: the blur ops read the convs' outputs in the plain form"""
    assert _full("batch").blur_summary(64, 256, 256) == {"launches": 4, "folded": 0}


def test_shape_inference_and_the_refusal_of_a_one_pixel_axis():
    """down: ceil(H / 2) x ceil(W / 2), refused when the geometry is planned if H < 2 or W < 2 (inside a generator the 7 x 7 stem's own reflection refuses such an
    image first); up: 2H x 2W from 1 x 1"""
    net = engine.HipNet(DEV, "f16")
    t = net.input(3)
    net.output_nchw(net.blur_resample(t))
    net.output_nchw(net.blur_resample(t, up=True))
    assert net.output_shapes(2, 5, 7) == [(2, 8, 3, 4), (2, 8, 10, 14)] and net.output_shapes(1, 2, 2) == [(1, 8, 1, 1), (1, 8, 4, 4)]
    for h, w in [(1, 7), (8, 1), (1, 1)]:
        with pytest.raises(ValueError, match="at least 2 x 2"):
            net.output_shapes(1, h, w)
        with pytest.raises(ValueError, match="at least 2 x 2"):
            net.blur_summary(1, h, w)
    up = engine.HipNet(DEV, "f16x3")
    up.output_nchw(up.blur_resample(up.input(3), up=True))
    assert up.output_shapes(3, 1, 1) == [(3, 8, 2, 2)] and up.blur_summary(3, 1, 4) == {"launches": 1, "folded": 0}


def test_norm_fusion_knob_switches_the_fold_off():
    """GDT_NORM_FUSION is latched at the first plan of a process: a child process per setting"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from gandtr_amd import engine\nfrom gandtr_amd.tools import synth\n"
            "net = engine.build_generator(synth.generator_state(0, 'instance', no_antialias=False, no_antialias_up=False), 'cuda:0', finalize=False)\n"
            "print(net.blur_summary(64, 256, 256), net.plan_summary(64, 256, 256)['norms_folded'])\n" % ROOT)
    env = dict(os.environ, GDT_NORM_FUSION="0")
    out = subprocess.run([sys.executable, "-c", code], env=env, check=True, capture_output=True, text=True).stdout
    assert out.strip() == "{'launches': 4, 'folded': 0} 0", out


HUB_PLAN = {"conv_launches": 24, "bottlenecks_fused": 0, "conv3x3_expand": 0, "chained_reduce": 0, "shortcuts_folded": 0, "norms_folded": 23, "pools_fused": 0,
            "direct_stem": 0, "transposed_fused": 2, "stride2_shift": 2, "dilated_convs": 0, "dilated_special_forms": 0, "head_launches": 0, "head_map_reads": 0,
            "conv4x4_launches": 0, "conv4x4t_launches": 0, "conv3x3_cat_launches": 0, "attention_launches": 0, "attention_map_reads": 0, "convt2x2_launches": 0}


def test_the_hub_generator_plans_as_before(monkeypatch):
    """the plan summary of the hub-configuration generator at (64, 256, 256), as recorded before the blur op existed; no counter was added to either table"""
    for k in ("GDT_NORM_FUSION", "GDT_CONV_CTF", "GDT_X3_NORM_FOLD", "GDT_CONV_HALO_X3", "GDT_CONV_HALO_X3_FORMS"):
        monkeypatch.delenv(k, raising=False)
    from gandtr_amd import _hip
    hub = engine.build_generator(synth.generator_state(0, "instance"), DEV, finalize=False)
    assert hub.plan_summary(64, 256, 256) == HUB_PLAN
    assert _hip.plan_count_more_names() == ("convt2x2_launches",) and len(_hip.plan_count_names()) == 19
