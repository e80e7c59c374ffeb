"""The local head on the device (csrc/local_head.hip): gdt_local_descriptors against float64 of the stored map, and the extraction functions of
cirnet.py (extract_ssl, extract_local_vectors, extract_local_features) on GeM-ResNet-18 / GeM-VGG16 with synthetic weights."""
import pytest
import torch

from gandtr_amd import engine
from gandtr_amd.components.model.network import cirnet
from gandtr_amd.tools import synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
KERNEL_CASES = [(1, 1, 1, 64), (2, 5, 7, 64), (3, 9, 4, 512), (1, 33, 31, 2048)]       # one position; ragged slabs of 32 and of 16 positions; several images


def _map(n, h, w, d, dtype):
    x = torch.relu(synth.synth_input(500 + d + h, (n, h, w, d), name="local.map")) * 3.0 + 0.01 * synth.synth_input(501, (n, h, w, d), name="local.map.low")
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("n,h,w,d", KERNEL_CASES)
def test_local_descriptors_kernel(cuda_device, n, h, w, d, dtype):
    """per element against float64 of the same stored map under (d + 2) 2^-24 relative + 2^-24 absolute: d roundings at most on any path of the sum
    of squares, halved by the square root, and the roundings of sqrtf, + eps and the division; the max-normalised attention adds the division"""
    x = _map(n, h, w, d, dtype)
    r = x.double()
    ss = (r * r).sum(-1)
    want = (r / (ss.sqrt() + float(torch.tensor(1e-6, dtype=torch.float32))).unsqueeze(-1)).permute(0, 3, 1, 2)
    watt = (ss + float(torch.tensor(1e-10, dtype=torch.float32))).sqrt()
    for nmax in (False, True):
        desc, att = engine.local_descriptors(x.to(cuda_device), 1e-6, nmax)
        assert desc.shape == (n, d, h, w) and att.shape == (n, h, w) and desc.dtype == att.dtype == torch.float32
        qd = float(((desc.cpu().double() - want).abs() / ((d + 2) * U * want.abs() + U)).max())
        ref_att = watt / watt.flatten(1).max(1)[0].view(-1, 1, 1) if nmax else watt
        qa = float(((att.cpu().double() - ref_att).abs() / ((d + (4 if nmax else 2)) * U * ref_att.abs() + U)).max())   # / max: the maximum's own error and the division
        print("local descriptors %s normalize_max %d: |d| / bound descriptors %.3f attention %.3f" % ((n, h, w, d), nmax, qd, qa))
        assert qd <= 1.0 and qa <= 1.0, (qd, qa)
        if nmax:
            assert float(att.flatten(1).max(1)[0].min()) == 1.0
    again, att2 = engine.local_descriptors(x.to(cuda_device), 1e-6, True)
    assert torch.equal(again, desc) and torch.equal(att2, att)


def test_local_descriptors_bad_arguments(cuda_device):
    with pytest.raises(ValueError):
        engine.local_descriptors(torch.zeros(1, 2, 2, 48, device=cuda_device))           # channels % 64
    with pytest.raises(ValueError):
        engine.local_descriptors(torch.zeros(1, 2, 2, 64))                               # not on the device


def _net(arch):
    torch.manual_seed(0)
    net = cirnet.init_cirnet(cir_architecture=arch, local_whitening=False, pooling="gem", regional=False, whitening=False, pretrained=False).eval()
    sd = synth.vgg16_state(0) if arch == "vgg16" else synth.resnet_basic_state(0)
    missing = net.load_state_dict({k: v for k, v in sd.items() if k.startswith("features.")}, strict=False)
    assert not missing.unexpected_keys
    return net


@pytest.mark.parametrize("arch", ["resnet18", "vgg16"])
def test_extract_ssl_f16x3_reconstructs_the_cpu_map(cuda_device, arch):
    """attention * descriptor gives the trunk's map back (x ||x|| / (||x|| + 1e-6)); compared with the CPU fp32 module's ``features`` within
    1e-5 max |map|, the exact mode's gate.  Every position enters with its own magnitude, so weak positions need no exclusion."""
    cpu = _net(arch)
    x = synth.synth_input(7, (1, 3, 64, 96))
    with torch.no_grad():
        fmap = cpu.features(x)[0]
        dev = _net(arch).to(cuda_device)
        dev.hip_precision = "f16x3"
        ssl = cirnet.extract_ssl(dev, x.to(cuda_device))
        desc, att = cirnet.local_forward(dev, x.to(cuda_device))
        ref = cirnet.extract_ssl(cpu, x)
    D = cpu.meta["out_channels"]
    assert ssl.is_cuda and ssl.shape == (D, fmap.shape[1] * fmap.shape[2]) == ref.shape
    assert torch.equal(ssl, desc[0].reshape(D, -1))
    back = (att[0].reshape(1, -1) * ssl).cpu().reshape(fmap.shape)
    err = float((back - fmap).abs().max() / fmap.abs().max())
    print("%s f16x3: max |attention * descriptor - map| / max |map| = %.2e" % (arch, err))
    assert err <= 1e-5, err


def test_extract_local_vectors_and_features(cuda_device):
    net = _net("resnet18").to(cuda_device)
    a, b = synth.synth_input(8, (3, 64, 96)), synth.synth_input(9, (1, 3, 96, 64))
    vecs = cirnet.extract_local_vectors(net, [a, b], None, None)
    with torch.no_grad():
        singles = [cirnet.extract_ssl(net, a.unsqueeze(0).to(cuda_device)), cirnet.extract_ssl(net, b.to(cuda_device))]
    assert [tuple(v.shape) for v in vecs] == [(512, 6), (512, 6)] and all(v.is_cuda for v in vecs)
    assert all(torch.equal(v, s) for v, s in zip(vecs, singles))
    with pytest.raises(NotImplementedError):
        cirnet.extract_local_vectors(net, [a, b], None, None, ms=[1, 0.5])
    feats = cirnet.extract_local_features(net, [a, b], None, None)
    assert len(feats) == 2 and tuple(feats[0][0][0].shape) == (512, 2, 3) and tuple(feats[1][1][0].shape) == (3, 2)
    assert torch.equal(feats[0][0][0].reshape(512, -1), vecs[0])
    # ... the structure Grouping.forward consumes
    from gandtr_amd.components.model.layers import grouping
    layer = grouping.LoadedCodebook(synth.synth_input(3, (5, 512)).to(cuda_device), "normresatt", "top-2", "softmax-2.0", "l2norm", "maxassatt", 1.0, 0,
                                    outputdim=512).to(cuda_device)
    with torch.no_grad():
        grouped, weights = layer(feats)
    assert tuple(grouped.shape) == (2, 5, 512) and tuple(weights.shape) == (2, 5) and bool(torch.isfinite(grouped).all())


def test_default_precision_equals_the_kernel_on_the_graphs_own_tap(cuda_device):
    """f16: the graph op's outputs are the standalone kernel's on the map the graph itself taps (output_nchw), bit for bit"""
    sd = synth.resnet_basic_state(0)
    net = engine.build_embedder(sd, cuda_device, head=("local", 1e-6, True), feature_tap=True)
    x = synth.synth_input(10, (2, 3, 96, 128)).to(cuda_device)
    outs = net.forward(x)
    tap = outs[net.feature_slot]
    desc, att = engine.local_descriptors(tap.permute(0, 2, 3, 1).contiguous().half(), 1e-6, True)
    assert tuple(outs[net.out_slot].shape) == (2, 512, 3, 4) and tuple(outs[net.attention_slot].shape) == (2, 3, 4)
    assert torch.equal(outs[net.out_slot], desc) and torch.equal(outs[net.attention_slot], att)
    plan = net.plan_summary(2, 96, 128)
    assert plan["head_launches"] == 2 and plan["head_map_reads"] == 1
