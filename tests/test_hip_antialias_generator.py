"""ResnetGenerator with CUT's anti-aliased sampling (no_antialias=False / no_antialias_up=False) on the device: the tiny net against the reference's fixtures
(tests/golden/make_antialias_golden.py) at every tap a device delivers, the mixed-flag and odd-size cases, one full-width net against the host mirror in float64, the
encoder-only graph, calculate_nce_loss, and the folded forward against GDT_NORM_FUSION=0.

Gates: the default mode ("f16c") rel = max |d| / max |ref| < 1e-3, the gate of test_hip_golden.py::test_generator_tiny_taps_vs_reference; "f16x3" the gates
tests/test_hip_models.py applies to the hub generator's exact mode: 1e-4 on the tiny net (test_generator_tiny_f16x3), 1e-5 on the full-width net
(test_generator_exact_mode_*).  Measured figures (MI355X) are in the docstrings of the tests."""
import os
import subprocess
import sys

import pytest
import torch

import blur_bound as bb
import blur_ref as br
from gandtr_amd import engine
from gandtr_amd.components.model.network import p2p_networks
from gandtr_amd.tools import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TINY_GATES = {"f16c": 1e-3, "f16x3": 1e-4}
CASE_FLAGS = {"down": (False, True), "up": (True, False), "odd": (False, False)}        # (no_antialias, no_antialias_up)


def rel(a, b):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _module(norm, flags, dev, precision, ngf=8, n_blocks=2):
    gen = p2p_networks.ResnetGenerator(3, 3, ngf=ngf, norm_layer=norm, n_blocks=n_blocks, no_antialias=flags[0], no_antialias_up=flags[1]).eval()
    gen.load_state_dict(synth.generator_state(0, norm, ngf=ngf, n_blocks=n_blocks, no_antialias=flags[0], no_antialias_up=flags[1]), strict=True)
    gen.hip_precision = precision
    return gen.to(dev)


def _against_fixture(gen, x, layers, golden, gate, label):
    """the output and every tap the fixture holds, through the module's HIP forward; prints the worst tap before asserting"""
    taps = sorted(t for t in golden if t not in (0, layers - 3))
    with torch.no_grad():
        out, feats = gen(x, layers=list(taps))
    rels = {t: rel(f.cpu()[:golden[t].shape[0]], golden[t]) for t, f in zip(taps, feats)}
    r_out = rel(out.cpu(), golden[layers - 1])
    worst = max(rels, key=rels.get)
    print("%s: output %.2e, worst tap %d %.2e (gate %.0e); taps %s" % (label, r_out, worst, rels[worst], gate, " ".join("%d:%.1e" % kv for kv in sorted(rels.items()))))
    assert r_out < gate, r_out
    for t, r in rels.items():
        assert r < gate, (t, r)


@pytest.mark.parametrize("precision", ["f16c", "f16x3"])
@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_tiny_net_every_tap_against_the_reference(cuda_device, norm, precision):
    """ngf 8, 2 blocks, both flags off, 2 x 3 x 32 x 32: taps 1 .. 21 and 23, 24 and the output.

    MEASURED on an MI355X, max |d| / max |ref|: InstanceNorm output 2.6e-6, worst tap 2.7e-6 (23, pre-tanh), the four sampling ops' outputs (7, 11, 14, 18) 4.3e-7,
    3.5e-7, 1.3e-6, 1.4e-6; BatchNorm output 1.1e-6 = worst tap.  The same figures in both modes: at this size the planner runs the f16c net on the exact-split
    kernels."""
    layers, golden = br.golden_taps("gen_tiny_aa_" + norm)
    gen = _module(norm, (False, False), cuda_device, precision)
    _against_fixture(gen, synth.synth_input(1, (2, 3, 32, 32), 1.0).to(cuda_device), layers, golden, TINY_GATES[precision], "tiny aa %s %s" % (norm, precision))


@pytest.mark.parametrize("precision", ["f16c", "f16x3"])
@pytest.mark.parametrize("tag", ["down", "up", "odd"])
def test_mixed_flags_and_odd_size_against_the_reference(cuda_device, tag, precision):
    """one flag at a time (Downsample with ConvTranspose2d; stride-2 convs with Upsample) and both flags off at 1 x 3 x 21 x 18 (maps 21 x 18, 11 x 9, 6 x 5, output 24 x 20)

    MEASURED on an MI355X, max |d| / max |ref|, output = worst tap: down 1.9e-6, up 1.8e-6, odd size 2.7e-6 (its sampling ops' outputs 4.3e-7, 5.6e-7, 1.1e-6, 1.5e-6);
    the same in both modes."""
    layers, golden = br.golden_taps("gen_tiny_aa_cases", tag + "_")
    x = synth.synth_input(1, (1, 3, 21, 18), 1.0) if tag == "odd" else synth.synth_input(1, (2, 3, 32, 32), 1.0)
    gen = _module("instance", CASE_FLAGS[tag], cuda_device, precision)
    _against_fixture(gen, x.to(cuda_device), layers, golden, TINY_GATES[precision], "aa case %s %s" % (tag, precision))


# ------------------------------------------------------------------------------------------------ full width
FULL = dict(ngf=64, n_blocks=2)
FULL_SHAPE = (2, 3, 64, 64)
FULL_TAPS = (4, 7, 8, 11, 13, 14, 15, 18, 19)      # raw convs, the four sampling ops' outputs, the blocks' output: none of them takes a fold away
_FULL = {}


def _full_reference():
    """the host mirror in float64 on the CPU (validated against the reference's fixtures in test_antialias_host.py), once: (input, output, taps, pre-tanh)"""
    if not _FULL:
        gen = p2p_networks.ResnetGenerator(3, 3, norm_layer="instance", no_antialias=False, no_antialias_up=False, **FULL).eval()
        gen.load_state_dict(synth.generator_state(0, "instance", no_antialias=False, no_antialias_up=False, **FULL), strict=True)
        x = synth.synth_input(3, FULL_SHAPE, 1.0)
        with torch.no_grad():
            out, feats = gen.double()(x.double(), layers=list(FULL_TAPS) + [23])
        _FULL.update(x=x, out=out, feats=dict(zip(FULL_TAPS, feats[:-1])), pre=feats[-1])
    return _FULL


def _full_net(dev, precision, taps=FULL_TAPS, **kw):
    sd = synth.generator_state(0, "instance", no_antialias=False, no_antialias_up=False, **FULL)
    return engine.build_generator(sd, dev, taps=taps, precision=precision, pre_tanh=True, **kw)


@pytest.mark.parametrize("precision,gate", [("f16c", 1e-3), ("f16x3", 1e-5)])
def test_full_width_net_against_the_host_mirror(cuda_device, precision, gate):
    """ngf 64, 2 blocks, InstanceNorm, 2 x 3 x 64 x 64: the smallest net with the 64-, 128- and 256-channel stride-1 convs and the three folds.  Prints the kernel
    variant of every conv (its route) and the time share of the blur ops.

    MEASURED on an MI355X, max |d| / max |ref|: f16x3 pre-tanh 1.2e-6, worst tap 1.2e-6 (14); f16c the same taps (1.2e-6: at batch 2 the convs run on the exact-split
    kernels, variants 300064 / 300128) and pre-tanh 4.3e-4 (the compensated head, 920007).  The four blur ops: 0.053 ms of 2.7 ms."""
    ref = _full_reference()
    net = _full_net(cuda_device, precision)
    assert net.blur_summary(*FULL_SHAPE[:1], *FULL_SHAPE[2:]) == {"launches": 4, "folded": 3}
    net.set_profiling(True)
    outs = net.forward(ref["x"].to(cuda_device))
    torch.cuda.synchronize()
    prof = net.profile()
    print("full-width aa %s conv variants: %s" % (precision, " ".join(str(v) for k, v, ms, fl in prof if k == 1)))
    total = sum(ms for k, v, ms, fl in prof)
    print("full-width aa %s: blur ops %s ms of %.3f ms" % (precision, " ".join("%.3f" % ms for k, v, ms, fl in prof if k == 12), total))
    rels = {t: rel(outs[net.tap_slots[t]].cpu(), ref["feats"][t]) for t in FULL_TAPS}
    pre = rel(outs[net.out_slot].cpu(), ref["pre"])
    worst = max(rels, key=rels.get)
    print("full-width aa %s: pre-tanh %.2e, worst tap %d %.2e (gate %.0e); taps %s" % (precision, pre, worst, rels[worst], gate,
                                                                                     " ".join("%d:%.1e" % kv for kv in sorted(rels.items()))))
    assert pre < gate, pre
    for t, r in rels.items():
        assert r < gate, (t, r)


# ------------------------------------------------------------------------------------------------ encoder-only graph, CUT's loss
NCE_LAYERS = [4, 7, 10, 14]


@pytest.mark.parametrize("precision", ["f16c", "f16x3", "f16"])
def test_encoder_only_graph_equals_the_full_graph_bitwise(cuda_device, precision):
    """forward(x, layers=[4, 7, 10, 14], encode_only=True) runs a graph that ends at tap 14 (the first Upsample's output with 2 blocks): the same taps as the full
    graph's, bit for bit -- the fold in front of index 7 is there in both, the norm in front of index 11 is tapped (10) in both"""
    gen = _module("instance", (False, False), cuda_device, precision, **FULL)
    x = synth.synth_input(3, FULL_SHAPE, 1.0).to(cuda_device)
    with torch.no_grad():
        enc = gen(x, layers=list(NCE_LAYERS), encode_only=True)
        out, feats = gen(x, layers=list(NCE_LAYERS))
    assert [tuple(f.shape) for f in enc] == [(2, 128, 64, 64), (2, 128, 32, 32), (2, 256, 32, 32), (2, 256, 32, 32)]
    assert len(feats) == 4 and all(torch.equal(a, b) for a, b in zip(enc, feats))
    nets = gen.__dict__["_hip_cache"]
    assert nets[("gen_enc", tuple(NCE_LAYERS), precision)].blur_summary(2, 64, 64) == {"launches": 3, "folded": 1}
    assert nets[("gen", tuple(NCE_LAYERS), precision)].blur_summary(2, 64, 64) == {"launches": 4, "folded": 2}


def test_calculate_nce_loss_runs_with_the_antialiased_generator(cuda_device):
    """CUT's contrastive loss with the generator it was designed around: layers 4, 7, 10, 14 of the anti-aliased net (widths 128, 128, 256, 256), in the exact mode
    against the same function on the CPU (the host mirror, the reference's torch ops) with the same patch positions.

    MEASURED on an MI355X: device 4.810483, CPU 4.810484."""
    from gandtr_amd.components.optim.criterion import patchnce
    gen = _module("instance", (False, False), "cpu", "f16x3", **FULL)
    widths = p2p_networks.generator_tap_channels(NCE_LAYERS, ngf=64, n_blocks=2, no_antialias=False, no_antialias_up=False)
    assert widths == [128, 128, 256, 256]
    netF = p2p_networks.PatchSampleF(input_nc=None, nce_layers=None, nc=64).eval()
    netF.create_mlp([torch.zeros(1, c, 1, 1) for c in widths], "cpu")
    netF.load_state_dict(synth.patchsample_state(90, widths, 64))
    crit = patchnce.initialize_patchnce_criterion({"loss": "multilayer_patchnce_loss", "batch_dim_for_bmm": 1, "nce_layers": "4,7,10,14", "num_patches": 32,
                                                   "temperature": 0.07, "weight": 1.0})
    src, tgt = synth.synth_input(5, FULL_SHAPE, 1.0, name="src"), synth.synth_input(5, FULL_SHAPE, 1.0, name="tgt")
    g = torch.Generator().manual_seed(0)
    ids = [torch.randperm(hw, generator=g)[:32] for hw in (64 * 64, 32 * 32, 32 * 32, 32 * 32)]
    with torch.no_grad():
        want = patchnce.calculate_nce_loss(crit, gen, netF, src, tgt, patch_ids=ids)
        gen, netF = gen.to(cuda_device), netF.to(cuda_device)
        got = patchnce.calculate_nce_loss(crit, gen, netF, src.to(cuda_device), tgt.to(cuda_device), patch_ids=ids)
    assert got.total.is_cuda and list(got.partial) == ["layer4", "layer7", "layer10", "layer14"]
    d = abs(float(got.total) - float(want.total))
    print("calculate_nce_loss, anti-aliased generator, f16x3: device %.6f, cpu %.6f, |d| = %.2e" % (float(got.total), float(want.total), d))
    assert torch.isfinite(got.total) and d < 1e-3 * abs(float(want.total))


# ------------------------------------------------------------------------------------------------ folded against GDT_NORM_FUSION=0
FUSION_TAPS = (4, 7, 11, 13, 14, 18)


def _fusion_run(path):
    """run in a child process with GDT_NORM_FUSION=0 (the knob is latched at a process's first plan): the three modes' outputs and taps, saved to ``path``; in "f16"
    also the stored normalised tensor the unfolded Downsample reads (tap 6)"""
    dev = torch.device("cuda:0")
    x = synth.synth_input(3, FULL_SHAPE, 1.0).to(dev)
    res = {}
    for precision in ("f16x3", "f16c", "f16"):
        taps = FUSION_TAPS + ((6,) if precision == "f16" and os.environ.get("GDT_NORM_FUSION") == "0" else ())
        net = _full_net(dev, precision, taps=taps)
        net.set_profiling(True)
        outs = net.forward(x)
        torch.cuda.synchronize()
        res[precision] = {"out": outs[net.out_slot].cpu(), "folded": net.blur_summary(2, 64, 64)["folded"], "variants": [v for k, v, ms, fl in net.profile() if k == 1],
                          **{t: outs[net.tap_slots[t]].cpu() for t in taps}}
    torch.save(res, path)


def test_folded_forward_against_norm_fusion_off(cuda_device, tmp_path):
    """The same net with every fold switched off (GDT_NORM_FUSION=0, child process): its norms store the normalised tensors and every consumer reads them back.
    "f16x3" and "f16c": fp32 tensors, and the fold applies the formula of the apply pass to the same fp32 values -- the raw conv in front of the first Downsample,
    the four blur ops' outputs and the blocks' output in between are compared bit for bit.  The pre-tanh output is NOT bit-identical (max |d| 6.0e-7 in f16x3,
    3.4e-5 in f16c): with the knob off the head conv's own fold goes too.  The kernel is the same (conv_head7.hip, variant 920007 in both runs), but its folded form
    stages x * rstd + (-mean * rstd), one fma, where the apply pass it replaces stores (x - mean) * rstd -- a difference of the head kernel's two forms that the hub
    generator has as well, not of the blur ops, whose last output (tap 18) is identical.  Both outputs are held to the float64 mirror under the mode's gate instead.  "f16": the unfolded net rounds the normalised tensor to fp16 before the blur and the folded one does not, so each
    Downsample output (tap 7) is held to its own float64 reference: the folded one to blur_bound.blur(raw tap 4, "relu"), the unfolded one to the plain bound on
    its stored tap 6.

    MEASURED on an MI355X: f16x3 and f16c -- taps 4, 7, 11, 13, 14, 18 bit-identical; f16 -- folded Downsample 0.322 of its bound (the epilogue-statistics bound),
    unfolded 0.998 of the plain bound."""
    path = str(tmp_path / "unfused.pt")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_hip_antialias_generator as t; t._fusion_run(%r)" % (os.path.dirname(HERE), HERE, path)
    subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GDT_NORM_FUSION="0"), check=True, timeout=600)
    unfused = torch.load(path)
    assert os.environ.get("GDT_NORM_FUSION") in (None, "1")
    _fusion_run(str(tmp_path / "fused.pt"))
    fused = torch.load(str(tmp_path / "fused.pt"))
    for precision in ("f16x3", "f16c"):
        a, b = fused[precision], unfused[precision]
        assert a["folded"] == 3 and b["folded"] == 0
        same = {k: torch.equal(a[k], b[k]) for k in FUSION_TAPS + ("out",)}
        diff = {k: float((a[k].double() - b[k].double()).abs().max()) for k in same}
        print("folded against GDT_NORM_FUSION=0, %s: bit-identical %s; max |d| %s" % (precision, same, {k: "%.2e" % v for k, v in diff.items()}))
        print("  conv variants folded %s, unfolded %s" % (a["variants"], b["variants"]))
        assert all(same[k] for k in FUSION_TAPS), (precision, same)
        gate = {"f16x3": 1e-5, "f16c": 1e-3}[precision]
        pre = _full_reference()["pre"]
        assert rel(a["out"], pre) < gate and rel(b["out"], pre) < gate, (precision, rel(a["out"], pre), rel(b["out"], pre))
    a, b = fused["f16"], unfused["f16"]
    assert a["folded"] == 3 and b["folded"] == 0
    bias = synth.generator_state(0, "instance", no_antialias=False, no_antialias_up=False, **FULL)["model.4.bias"].view(1, -1, 1, 1)
    raw = a[4] - bias                       # the tap adds the conv's bias, which the bias-free graph never had; InstanceNorm is invariant to it
    bb.assert_within(a[7], bb.blur(raw, False, "relu", out_f32=False, fused=br.fused_statistics(raw.shape)), "f16 folded Downsample against float64 of the raw tap")
    bb.assert_within(b[7], bb.blur(b[6], False, None, out_f32=False), "f16 unfolded Downsample against float64 of its stored input")
