"""ResNet-18 / ResNet-34 (BasicBlock trunks) on the host: the restated architecture against torchvision's published counts and key names, init_network and its
three wrappers, the synthetic state dict, the CPU forward -- and what the planner decides for the device graph (host logic: no device call before finalize).

The fused BasicBlock route (conv3x3_basic.hip) is OFF by default: the whole-forward measurement of tools/resnet_basic_bench.py is a tie / loss (DESIGN.md section 4,
profiles/resnet_basic_1gpu.json).  So with GDT_CONV_BASIC unset both nets plan 0 fused blocks at 32 x 3 x 1024^2, and 2 (ResNet-18: layer1's two blocks) / 3
(ResNet-34) with GDT_CONV_BASIC=1."""
import pytest
import torch

from gandtr_amd import engine
from gandtr_amd.components.model import network as registry
from gandtr_amd.components.model.network import backbones, cirnet
from gandtr_amd.tools import synth

DEV = "cuda:0"        # only recorded; no device call happens before finalize()
NETS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}
BASE = dict(local_whitening=False, pooling="gem", regional=False, whitening=False, pretrained=False)
BIG = (32, 1024, 1024)


@pytest.mark.parametrize("arch,params,entries", [("resnet18", 11689512, 122), ("resnet34", 21797672, 218)])
def test_architecture_has_torchvisions_counts_and_names(arch, params, entries):
    m = backbones.ARCHITECTURES[arch]()
    sd = m.state_dict()
    assert sum(p.numel() for p in m.parameters()) == params and len(sd) == entries
    assert "layer1.0.conv1.weight" in sd and "layer2.0.downsample.1.running_var" in sd
    assert not [k for k in sd if k.startswith("layer1.0.downsample")]
    for li in (2, 3, 4):                                            # a projection only where stride or width change: the first block of layers 2-4
        assert "layer%d.0.downsample.0.weight" % li in sd and not [k for k in sd if k.startswith("layer%d.1.downsample" % li)]
    blk = m.layer2[0]
    assert type(blk) is backbones.BasicBlock and blk.expansion == 1
    assert [n for n, _ in blk.named_children()] == ["conv1", "bn1", "relu", "conv2", "bn2", "downsample"]
    assert blk.conv1.stride == (2, 2) and blk.conv2.stride == (1, 1) and blk.downsample[0].stride == (2, 2) and blk.downsample[0].kernel_size == (1, 1)
    assert m.layer1[0].downsample is None and m.fc.in_features == 512
    assert backbones.resnet101().fc.in_features == 2048             # (the Bottleneck nets are what they were)


@pytest.mark.parametrize("arch", sorted(NETS))
def test_init_network_and_the_registry(arch):
    net = cirnet.init_network(dict(BASE, architecture=arch))
    assert net.meta["outputdim"] == 512 and net.meta["architecture"] == arch and cirnet.OUTPUT_DIM[arch] == 512
    model = registry.initialize_model(dict(BASE, architecture="cirnet", cir_architecture=arch))
    assert model.meta["outputdim"] == 512 and model.meta["out_channels"] == 512
    assert arch in cirnet.ImageRetrievalNet.HIP_TRUNKS
    with pytest.raises(ValueError):
        cirnet.init_network(dict(BASE, architecture="alexnet9"))


@pytest.mark.parametrize("arch", sorted(NETS))
def test_synthetic_state_loads_strictly_and_the_cpu_forward_is_unit_norm(arch):
    sd = synth.resnet_basic_state(0, blocks=NETS[arch])
    assert "features.4.0.conv1.weight" in sd and "features.5.0.downsample.1.running_var" in sd and "pool.p" in sd
    assert not [k for k in sd if k.startswith("features.4.0.downsample") or ".conv3." in k]
    assert float(sd["features.4.0.bn1.running_mean"].abs().max()) > 0 and float((sd["features.4.0.bn1.running_var"] - 1).abs().max()) > 0      # non-trivial statistics
    net = cirnet.init_network(dict(BASE, architecture=arch)).eval()
    net.load_state_dict(sd, strict=True)
    x = synth.synth_input(3, (2, 3, 37, 45))
    with torch.no_grad():
        out = net(x)
    assert tuple(out.shape) == (512, 2) and bool(torch.isfinite(out).all())
    assert float((out.norm(dim=0) - 1).abs().max()) < 1e-5
    assert engine.embedder_arch(sd) == "resnet"


def test_inchan_and_attention_wrappers_construct_and_run():
    params = dict(BASE, cir_architecture="resnet18")
    one = cirnet.init_cirnet_inchan({"channels": 1, "preprocessing": None}, **dict(params)).eval()
    assert one.meta["in_channels"] == 1 and one.features[0].weight.shape[1] == 1
    att = cirnet.init_cirnet_attention({"type": "l2norm", "normalize_max": True}, **dict(params)).eval()
    with torch.no_grad():
        a = one(synth.synth_input(4, (2, 1, 37, 45)))
        b = att(synth.synth_input(4, (2, 3, 37, 45)))
    for out in (a, b):
        assert tuple(out.shape) == (512, 2) and float((out.norm(dim=0) - 1).abs().max()) < 1e-5


@pytest.mark.parametrize("arch,identity_blocks", [("resnet18", 2), ("resnet34", 3)])
def test_planner_counts_fused_basic_blocks(arch, identity_blocks, monkeypatch):
    """measured default OFF: 0 with the knob unset, layer1's identity blocks (2 / 3) with GDT_CONV_BASIC=1; 0 with the knob at 0 and in f16x3; the layout
    of a geometry does not depend on the route"""
    monkeypatch.delenv("GDT_CONV_BASIC", raising=False)
    sd = synth.resnet_basic_state(0, blocks=NETS[arch])
    net = engine.build_embedder(sd, DEV, finalize=False)
    assert net.basic_blocks_fused(*BIG) == 0
    launches, ws = net.plan_summary(*BIG)["conv_launches"], net.workspace_bytes(*BIG)
    assert launches == 1 + 2 * sum(NETS[arch]) + 3                  # stem, two convs per block, three projections
    monkeypatch.setenv("GDT_CONV_BASIC", "1")
    assert net.basic_blocks_fused(*BIG) == identity_blocks
    assert net.plan_summary(*BIG)["conv_launches"] == launches - identity_blocks and net.workspace_bytes(*BIG) == ws
    assert net.basic_blocks_fused(2, 160, 192) == 0                 # 2 x 3 x 3 patches: below the tile threshold
    monkeypatch.setenv("GDT_CONV_BASIC", "2")
    assert net.basic_blocks_fused(*BIG) == identity_blocks and net.basic_blocks_fused(2, 160, 192) == identity_blocks
    assert engine.build_embedder(sd, DEV, precision="f16x3", finalize=False).basic_blocks_fused(*BIG) == 0
    monkeypatch.setenv("GDT_CONV_BASIC", "0")
    assert net.basic_blocks_fused(*BIG) == 0
    assert engine.build_embedder(sd, DEV, precision="f16x3", finalize=False).basic_blocks_fused(*BIG) == 0


def test_existing_nets_plan_as_before(monkeypatch):
    """no BasicBlock in ResNet-101 (Bottlenecks) or in the BatchNorm generator at ngf 16 (64-wide blocks, but reflect padding and no final ReLU): count 0 and the
    whole plan summary equal with the knob at 0 and at 2"""
    r101 = engine.build_embedder(synth.resnet101_state(0), DEV, finalize=False)
    gen = engine.build_generator(synth.generator_state(0, "batch", ngf=16), DEV, precision="f16", finalize=False)
    plans = {}
    for knob in ("0", "2"):
        monkeypatch.setenv("GDT_CONV_BASIC", knob)
        assert r101.basic_blocks_fused(*BIG) == 0 and gen.basic_blocks_fused(64, 256, 256) == 0
        plans[knob] = (r101.plan_summary(*BIG), gen.plan_summary(64, 256, 256), r101.workspace_bytes(*BIG), gen.workspace_bytes(64, 256, 256))
    assert plans["0"] == plans["2"]
    assert plans["0"][0]["bottlenecks_fused"] == 6 and plans["0"][0]["conv3x3_expand"] == 22        # (test_planner_cpu.py's figures)
