"""The PatchGAN discriminator mirror and the adversarial criterion on the host (no GPU): registry, module tree, fp32 logits and losses against the
fixture the reference wrote (tests/golden/make_discriminator_golden.py), the unsupported configurations, the planner's choice of the 4x4 patch kernel."""
import os

import numpy as np
import pytest
import torch

from gandtr_amd.tools import synth

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "discriminator.npz"))
N_CASES = int(GOLD["n_cases"])
# train_hedngan.yml:46-58, the discriminator_Y block
HEDNGAN_DISCRIMINATOR = {"type": "SingleNetwork",
                         "model": {"architecture": "official_p2p_discriminator", "no_antialias": True, "input_nc": 3, "norm_layer": "batch"},
                         "initialize": {"weights": "kaiming_p2p", "seed": 0},
                         "runtime": {"wrappers": "", "data": {}}}


def case(i):
    """(mirror in eval mode with the fixture's seeded weights, seeded input, fixture prefix)"""
    from gandtr_amd.components.model.network import p2p_networks
    p = "c%d_" % i
    ndf, n_layers, wseed, xseed = (int(v) for v in GOLD[p + "cfg"])
    norm = str(GOLD[p + "norm"])
    model = p2p_networks.NLayerDiscriminator(3, ndf=ndf, n_layers=n_layers, norm_layer=norm).eval()
    model.load_state_dict(synth.discriminator_state(wseed, norm, ndf=ndf, n_layers=n_layers, gain=float(GOLD["gain"])))
    x = synth.synth_input(xseed, tuple(int(v) for v in GOLD[p + "shape"]), 1.0)
    return model, x, p


def test_registry_label_and_mdir_shim_resolve_to_the_mirror():
    from gandtr_amd.components.model import network as registry
    from gandtr_amd.components.model.network import p2p_networks
    assert registry.MODEL_LABELS["official_p2p_discriminator"] is p2p_networks.NLayerDiscriminator
    import mdir.components.model.network as ref_registry
    from mdir.components.model.network import p2p_networks as shim_p2p
    assert ref_registry.MODEL_LABELS["official_p2p_discriminator"] is shim_p2p.NLayerDiscriminator is p2p_networks.NLayerDiscriminator
    model = registry.initialize_model({"architecture": "official_p2p_discriminator", "no_antialias": True, "input_nc": 3, "norm_layer": "batch"})
    assert model.meta == {"in_channels": 3, "out_channels": 1}
    import copy
    from gandtr_amd.learning import network as learning
    net = learning.initialize_network(copy.deepcopy(HEDNGAN_DISCRIMINATOR), "cpu")
    assert isinstance(net.model, p2p_networks.NLayerDiscriminator) and net.meta["out_channels"] == 1
    with torch.no_grad():
        y = net.eval()(synth.synth_input(1, (1, 3, 64, 64), 1.0))
    assert tuple(y.shape) == (1, 1, 6, 6)
    assert tuple(net.model.forward_multi(synth.synth_input(1, (1, 3, 64, 64), 1.0)).shape) == (1, 1, 6, 6)


def test_adversarial_module_and_unchanged_criteria_registry():
    from gandtr_amd.components.optim import criterion
    from gandtr_amd.components.optim.criterion import adversarial
    import mdir.components.optim.criterion.adversarial as shim
    assert shim is adversarial
    assert set(criterion.CRITERIA) == {"contrastive", "triplet"}
    with pytest.raises(NotImplementedError):
        criterion.initialize_criterion({"loss": "discriminator_loss", "criterion": {"loss": "mse"}})
    crit = adversarial.initialize_adversarial_criterion({"loss": "discriminator_loss", "criterion": {"loss": "mse"}})
    assert isinstance(crit, adversarial.DiscriminatorLoss) and crit.kind == "mse"
    assert adversarial.initialize_adversarial_criterion(None) is None
    with pytest.raises(NotImplementedError):
        adversarial.DiscriminatorLoss(criterion={"loss": "l1"})
    with pytest.raises(NotImplementedError):
        adversarial.patch_scores(torch.zeros(1, 1, 2, 2), "hinge")
    with pytest.raises(ValueError):
        adversarial.patch_scores(torch.zeros(1, 3, 2, 2), "mse")


@pytest.mark.parametrize("i", range(N_CASES))
def test_state_dict_keys_and_shapes_are_the_references(i):
    model, _, p = case(i)
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in GOLD[p + "keys"]]
    assert [list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()] == GOLD[p + "shapes"].tolist()


def test_parameter_count():
    from gandtr_amd.components.model.network import p2p_networks
    model = p2p_networks.NLayerDiscriminator(3, ndf=64, n_layers=3, norm_layer="instance")
    assert sum(q.numel() for q in model.parameters()) == int(GOLD["param_count_ndf64_l3_instance"]) == 2764737


@pytest.mark.parametrize("i", range(N_CASES))
def test_cpu_forward_reproduces_the_reference_logits(i):
    """fp32 against fp32: 1e-5 of the map's range"""
    model, x, p = case(i)
    ref = torch.from_numpy(GOLD[p + "logits"])
    with torch.no_grad():
        y = model(x)
    assert y.shape == ref.shape
    rel = float((y - ref).abs().max() / ref.abs().max())
    print("case %d: max|d| / max|ref| = %.3e" % (i, rel))
    assert rel <= 1e-5


@pytest.mark.parametrize("i", range(N_CASES))
def test_discriminator_loss_reproduces_the_reference_with_real_0_fake_1(i):
    from gandtr_amd.components.optim.criterion import adversarial
    p = "c%d_" % i
    y = torch.from_numpy(GOLD[p + "logits"])
    crit = adversarial.DiscriminatorLoss(criterion={"loss": "mse"})
    real, fake = crit(y, True, "cpu"), crit.forward(y, False, "cpu")
    # the reference's quirk: a real target is 0, a fake target is 1
    assert float(real.total) == pytest.approx(float((y.double() ** 2).mean()), rel=1e-6)
    assert float(fake.total) == pytest.approx(float(((y.double() - 1) ** 2).mean()), rel=1e-6)
    # the stored values are the reference's fp32 means: a few fp32 roundings of the sum
    assert float(real.total) == pytest.approx(float(GOLD[p + "loss_real"]), rel=1e-5)
    assert float(fake.total) == pytest.approx(float(GOLD[p + "loss_fake"]), rel=1e-5)
    assert real.total.dtype == torch.float32 and real.partial == {}
    # the list (multiscale) form sums the parts and names them from the end
    both = crit([y, y[:1]], True, "cpu")
    assert set(both.partial) == {"layer1", "layer0"}
    assert float(both.total) == pytest.approx(float(real.total) + float((y[:1].double() ** 2).mean()), rel=1e-6)
    assert float(both.partial["layer1"]) == float(real.total)
    s = adversarial.patch_scores(y, "bce_with_logits")
    want = torch.nn.functional.binary_cross_entropy_with_logits(y.double(), torch.ones_like(y.double()), reduction="none").reshape(y.shape[0], -1).mean(dim=1)
    assert torch.allclose(s.loss_target1, want, rtol=1e-12, atol=0)
    assert torch.allclose(s.mean_logit, y.double().reshape(y.shape[0], -1).mean(dim=1), rtol=1e-12, atol=1e-15)


def test_unsupported_configurations_raise():
    from gandtr_amd.components.model.network import p2p_networks
    with pytest.raises(NotImplementedError):
        p2p_networks.NLayerDiscriminator(3, no_antialias=False)
    with pytest.raises(NotImplementedError):
        p2p_networks.NLayerDiscriminator(3, kw=3)
    with pytest.raises(NotImplementedError):
        p2p_networks.NLayerDiscriminator(3, norm_layer="group")


def test_builder_plans_the_patch_kernel_for_layers_2_to_4(monkeypatch):
    """host logic only (gdt_net_plan_summary): the three middle convs of the ndf = 64 net run on conv4x4_halo.hip, none with the knob off, none in f16x3; the
    generator's plan does not know the new counter"""
    from gandtr_amd import engine
    monkeypatch.delenv("GDT_CONV4X4_HALO", raising=False)
    for norm in ("instance", "batch"):
        net = engine.build_discriminator(synth.discriminator_state(0, norm), "cuda:0", finalize=False)
        assert net.output_shapes(2, 256, 256) == [(2, 1, 30, 30)]
        # 2 * 16 * (128^2 * 3 * 64 + 64^2 * 64 * 128 + 32^2 * 128 * 256 + 31^2 * 256 * 512 + 30^2 * 512): ~400 GFLOP behind a 64 x 256^2 batch
        assert net.flops(1, 256, 256) / 1e9 == pytest.approx(6.2936, abs=0.001)
        assert net.conv4x4_launches(64, 256, 256) == 3 and net.conv4x4_launches(2, 40, 52) == 3
        assert net.plan_summary(64, 256, 256)["conv_launches"] == 5 and net.plan_summary(64, 256, 256)["norms_folded"] == 0
        monkeypatch.setenv("GDT_CONV4X4_HALO", "0")
        assert net.conv4x4_launches(64, 256, 256) == 0
        monkeypatch.delenv("GDT_CONV4X4_HALO")
        assert net.conv4x4_launches(64, 256, 256) == 3
    exact = engine.build_discriminator(synth.discriminator_state(0, "instance"), "cuda:0", precision="f16x3", finalize=False)
    assert exact.conv4x4_launches(64, 256, 256) == 0
    small = engine.build_discriminator(synth.discriminator_state(0, "instance", ndf=16, n_layers=2), "cuda:0", finalize=False)
    assert small.conv4x4_launches(2, 40, 52) == 0
    gen = engine.build_generator(synth.generator_state(0, "instance", ngf=16, n_blocks=2), "cuda:0", precision="f16", finalize=False)
    assert gen.conv4x4_launches(2, 64, 64) == 0
    with pytest.raises(NotImplementedError):
        engine.build_discriminator(synth.discriminator_state(0, "instance"), "cuda:0", precision="f16c", finalize=False)
    with pytest.raises(NotImplementedError):          # 48 -> 96 -> 192 channels: no power of two for the InstanceNorm kernels
        engine.build_discriminator(synth.discriminator_state(0, "instance", ndf=48), "cuda:0", finalize=False)
    net = engine.HipNet("cuda:0")
    t = net.input(3)
    with pytest.raises(ValueError):
        net.conv(t, synth._normal(0, "w", (16, 3, 4, 4)), stride=2, pad=1, leaky=1.5)          # slope outside (0, 1)
    a = net.conv(t, synth._normal(0, "w", (16, 3, 4, 4)), stride=2, pad=1, leaky=0.2)
    with pytest.raises(ValueError):
        net.instance_norm(a, leaky=-0.1)
    with pytest.raises(ValueError):
        engine.HipNet("cuda:0", precision="f16c").conv(t, synth._normal(0, "w", (16, 3, 4, 4)), leaky=0.2)
