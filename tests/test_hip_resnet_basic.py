"""GeM-ResNet-18 / -34 (BasicBlock trunks) on the device against the repository's own host module on the CPU in fp32 (init_network with the synthetic state
dict loaded strictly; the oracle has no BasicBlock): the graph of build_embedder in f16 -- layer by layer, with the fused BasicBlock kernel forced
(GDT_CONV_BASIC=2, variant 936064) and with it off -- and in f16x3, the module path (init_cirnet(...).to(cuda)), forward_many over a three-level pyramid on
side streams, and the refusal of an unlisted trunk.

Gates: the project's descriptor gates in f16 (|d|_inf < 1e-3, cosine > 0.9999 per image; tests/test_hip_golden.py), 2e-5 in f16x3 (test_embedder_f16x3).

MEASURED (MI355X), worst over the three inputs (max |d|, min cosine):
    resnet18 f16   knob unset / 0: 9.70e-05, 0.9999999   GDT_CONV_BASIC=2: 7.95e-05, 0.9999999
    resnet34 f16   knob unset / 0: 1.44e-04, 0.9999998   GDT_CONV_BASIC=2: 1.39e-04, 0.9999998
    resnet18 f16x3 4.47e-08 (1 - cosine 2.8e-14)         resnet34 f16x3 5.32e-08 (1 - cosine 3.6e-14)
    init_cirnet resnet18, gem + whitening, module path f16: 3.81e-05, 1.0000000
"""
import pytest
import torch

from gandtr_amd import engine
from gandtr_amd.components.model import network as registry
from gandtr_amd.components.model.network import cirnet
from gandtr_amd.tools import synth

pytestmark = pytest.mark.gpu

FUSED = 936064
NETS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}
INPUTS = [(2, 3, 160, 192), (1, 3, 250, 333), (3, 3, 97, 64)]
BASE = dict(local_whitening=False, pooling="gem", regional=False, whitening=False, pretrained=False)
GATE_ABS, GATE_COS, GATE_X3 = 1e-3, 0.9999, 2e-5
_REFS = {}


def _input(i):
    return synth.synth_input(40 + i, INPUTS[i])


def _reference(arch, i):
    """the CPU fp32 host module's descriptors [N][512] of input i, computed once per (net, input)"""
    if (arch, i) not in _REFS:
        net = cirnet.init_network(dict(BASE, architecture=arch)).eval()
        net.load_state_dict(synth.resnet_basic_state(0, blocks=NETS[arch]), strict=True)
        with torch.no_grad():
            _REFS[(arch, i)] = net(_input(i)).t().contiguous()
    return _REFS[(arch, i)]


def _errors(got, ref):
    got, ref = got.detach().cpu().double(), ref.double()
    return float((got - ref).abs().max()), float(torch.nn.functional.cosine_similarity(got, ref, dim=1).min())


@pytest.mark.parametrize("arch", sorted(NETS))
def test_embedder_f16(cuda_device, arch, monkeypatch):
    net = engine.build_embedder(synth.resnet_basic_state(0, blocks=NETS[arch]), cuda_device)
    net.set_profiling(True)
    identity_blocks = NETS[arch][0]
    for knob in (None, "2", "0"):                                   # read when a geometry is planned: every forward
        if knob is None:
            monkeypatch.delenv("GDT_CONV_BASIC", raising=False)
        else:
            monkeypatch.setenv("GDT_CONV_BASIC", knob)
        for i in range(len(INPUTS)):
            got = net.forward(_input(i).to(cuda_device))[net.out_slot]
            torch.cuda.synchronize()
            ran = [v for k, v, ms, fl in net.profile() if k == 1]
            assert ran.count(FUSED) == (identity_blocks if knob == "2" else 0), (knob, ran)      # (unset: the measured default, off)
            err, cos = _errors(got, _reference(arch, i))
            print("%s f16 GDT_CONV_BASIC=%s %s: max|d| %.3e  min cosine %.7f" % (arch, knob, INPUTS[i], err, cos))
            assert tuple(got.shape) == (INPUTS[i][0], 512)
            assert err < GATE_ABS and cos > GATE_COS, (arch, knob, i, err, cos)


@pytest.mark.parametrize("arch", sorted(NETS))
def test_embedder_f16x3(cuda_device, arch, monkeypatch):
    monkeypatch.setenv("GDT_CONV_BASIC", "2")                       # (no f16x3 form: nothing fuses)
    net = engine.build_embedder(synth.resnet_basic_state(0, blocks=NETS[arch]), cuda_device, precision="f16x3")
    net.set_profiling(True)
    for i in range(len(INPUTS)):
        got = net.forward(_input(i).to(cuda_device))[net.out_slot]
        torch.cuda.synchronize()
        assert FUSED not in [v for k, v, ms, fl in net.profile() if k == 1]
        err, cos = _errors(got, _reference(arch, i))
        print("%s f16x3 %s: max|d| %.3e  1 - min cosine %.3e" % (arch, INPUTS[i], err, 1.0 - cos))
        assert err < GATE_X3, (arch, i, err)


def test_module_path_equals_its_cpu_forward(cuda_device, monkeypatch):
    monkeypatch.delenv("GDT_CONV_BASIC", raising=False)
    torch.manual_seed(1000)
    net = cirnet.init_cirnet(cir_architecture="resnet18", **dict(BASE, whitening=True)).eval()
    state = synth.resnet_basic_state(0)
    net.load_state_dict(dict(net.state_dict(), **{k: v for k, v in state.items()}), strict=True)      # (the whitening layer keeps its seeded initialisation)
    x = _input(0)
    with torch.no_grad():
        ref = net(x)
        out = net.to(cuda_device)(x.to(cuda_device))
    assert tuple(out.shape) == (512, 2)
    err, cos = _errors(out.t(), ref.t())
    print("init_cirnet resnet18 gem + whitening, module path f16: max|d| %.3e  min cosine %.7f" % (err, cos))
    assert err < GATE_ABS and cos > GATE_COS, (err, cos)


def test_forward_many_equals_the_levels_one_by_one(cuda_device, monkeypatch):
    """a three-level pyramid with the fused BasicBlocks: forward_many (one side stream per level) against forward level by level, bit for bit"""
    monkeypatch.setenv("GDT_CONV_BASIC", "2")
    net = engine.build_embedder(synth.resnet_basic_state(0), cuda_device)
    x = _input(0).to(cuda_device)
    levels = [(x, None), (x, 2 ** -0.5), (x, 0.5)]
    assert [net.basic_blocks_fused(2, *net.resized_size(160, 192, s)) for _, s in levels] == [2, 2, 2]
    many = net.forward_many(levels)
    torch.cuda.synchronize()
    single = [net.forward(xx, scale=s) for xx, s in levels]
    torch.cuda.synchronize()
    for a, b in zip(many, single):
        assert torch.equal(a[net.out_slot], b[net.out_slot])


def test_an_unlisted_trunk_still_raises():
    with pytest.raises(ValueError):
        registry.initialize_model(dict(BASE, architecture="cirnet", cir_architecture="alexnet9"))
    with pytest.raises(ValueError):
        cirnet.init_network(dict(BASE, architecture="densenet121"))
