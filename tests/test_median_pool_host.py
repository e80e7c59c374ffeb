"""The geometric-median (Weiszfeld) pooling of the retrieval embedder on the host (no GPU): the torch mirror of the reference's GeometricMedianWeiszfeld /
WeightedGeometricMedianWeiszfeld and of init_cirnet* with the dict-valued pooling against what the reference itself produced (tests/golden/median_pool.npz,
written by tests/golden/make_median_pool_golden.py), against the float64 restatement (tests/median_ref.py), the refusals, the C ABI's argument errors and the
planner's counts for the median head.

The mirror runs the reference's fp32 op sequence image by image, and on the host that wrote the fixture its outputs EQUAL the reference's; what is asserted is
4 * 2^-24 of the vector's largest entry, which leaves another host's differently blocked sums their last bit (equality is printed per run)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_descriptor_heads_golden as H                        # noqa: E402  (seeded maps; imports no reference code)
import make_median_pool_golden as M                             # noqa: E402  (seeds, case lists; imports no reference code)
import median_ref                                               # noqa: E402
from gandtr_amd import _hip, engine                             # noqa: E402
from gandtr_amd.components.model import layers                  # noqa: E402
from gandtr_amd.components.model.network import cirnet          # noqa: E402
from gandtr_amd.tools import synth                              # noqa: E402

EPS24 = 2.0 ** -24
INITS = {"cirnet": cirnet.init_cirnet, "att": cirnet.init_cirnet_attention, "inchan": cirnet.init_cirnet_inchan}
BASE = dict(cir_architecture="vgg16", local_whitening=False, regional=False, whitening=False, pretrained=False)
GM = layers.pooling.GeometricMedianWeiszfeld
WGM = layers.pooling.WeightedGeometricMedianWeiszfeld


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "median_pool.npz"))


def ref_gate(h, w, d, ref):
    """first-order bound of the last weighted mean (two h*w-term fp32 sums in any order) plus a weight's d-term sum, root and division"""
    return (h * w + d + 8) * EPS24 * float(ref.abs().max())


def test_registry_and_alias():
    import mdir                                                  # noqa: F401
    from mdir.components.model.layers import pooling as alias_pooling
    assert alias_pooling is layers.pooling
    assert layers.pooling.POOLINGS == {"GeometricMedianWeiszfeld": GM}
    for layer in (GM(3, False), WGM(2, True, layers.attention.L2NormAttention(True))):
        assert not list(layer.parameters()) and not list(layer.buffers())
    assert GM(3, True).iterations == 3 and GM(3, True).intermediate_gradients is True


@pytest.mark.parametrize("si", range(len(H.LAYER_SIZES)), ids=["%dx%d" % s for s in H.LAYER_SIZES])
def test_layers_against_the_reference_and_float64(golden, si):
    h, w = H.LAYER_SIZES[si]
    equal = True
    for kind in H.LAYER_KINDS:
        x = H.layer_map(si, kind)
        cases = [("gm_%d_%s_%d" % (si, kind, it), GM(it, False), it, None) for it in M.LAYER_ITERATIONS]
        for nmax in (False, True):
            att = layers.attention.L2NormAttention(nmax)
            prior = torch.stack([att(x[i:i + 1]).reshape(x.shape[2:]) for i in range(x.size(0))])
            cases += [("wgm_%d_%s_%d_%d" % (si, kind, nmax, it), WGM(it, False, att), it, prior) for it in M.WEIGHTED_ITERATIONS]
        for key, layer, it, prior in cases:
            with torch.no_grad():
                got = layer(x)
            assert got.shape == (2, H.LAYER_D, 1, 1) and got.dtype == torch.float32
            got, ref = got.flatten(1), torch.from_numpy(golden[key])
            equal = equal and torch.equal(got, ref)
            assert float((got - ref).abs().max()) <= 4 * EPS24 * float(ref.abs().max()), key
            ref64 = median_ref.nchw(x, it, prior=prior)
            assert float((got.double() - ref64).abs().max()) <= ref_gate(h, w, H.LAYER_D, ref64), key
    print("%dx%d: the mirror %s the reference's outputs" % (h, w, "equals" if equal else "is within 4 * 2^-24 of"))


def test_zero_iterations_is_the_mean_and_the_median_is_robust(golden):
    x = M.outlier_map()
    with torch.no_grad():
        mean, med = GM(0, False)(x), GM(5, False)(x)
    assert float((mean - x.mean(dim=(2, 3), keepdim=True)).abs().max()) <= 1e-4
    for it, got in ((0, mean), (5, med)):
        ref = torch.from_numpy(golden["outlier_%d" % it])
        assert float((got.flatten(1) - ref).abs().max()) <= 4 * EPS24 * float(ref.abs().max())
    assert float(mean.max()) > 15.0 and float(med.max()) < 0.1 * float(mean.max())      # one position at 1000 moves the mean, not the median


def test_an_image_does_not_depend_on_the_batch():
    x = torch.relu(synth.synth_input(21, (3, 128, 9, 13)))
    x[1] *= 7.0
    att = layers.attention.L2NormAttention(True)
    for layer in (GM(0, False), GM(3, False), WGM(3, False, att)):
        with torch.no_grad():
            whole = layer(x)
            single = torch.cat([layer(x[i:i + 1]) for i in range(3)])
        assert torch.equal(whole, single)
    ref = median_ref.nchw(x, 3)
    assert torch.equal(ref[1:2], median_ref.nchw(x[1:2], 3))


def test_init_with_the_dict_pooling():
    given = {"type": "GeometricMedianWeiszfeld", "iterations": 4, "intermediate_gradients": True}
    kept = dict(given)
    net = cirnet.init_cirnet(pooling=given, **BASE)
    assert given == kept                                             # the caller's dict is left alone (the reference pops its type)
    assert type(net) is cirnet.CirRetrievalNet and type(net.pool) is GM and net.pool.iterations == 4 and net.pool.intermediate_gradients is True
    assert net.meta["pooling"] == kept and net.meta["pooling"] is not given and net.meta["regional"] is False
    assert [k for k in net.state_dict() if not k.startswith("features.")] == []
    assert "GeometricMedianWeiszfeld" in repr(net) and "'iterations': 4" in net.meta_repr()
    again = cirnet.init_cirnet(**{k: net.meta[k] for k in ("local_whitening", "pooling", "regional", "whitening")}, cir_architecture="vgg16",
                               pretrained=False)                     # a net rebuilt from its own meta
    assert type(again.pool) is GM and again.pool.iterations == 4 and again.meta["pooling"] == kept
    groups = net.parameter_groups({"lr": 0.5})
    assert len(groups) == 2 and list(groups[1]["params"]) == [] and groups[1]["lr"] == 5.0 and groups[1]["weight_decay"] == 0
    assert net._hip_head() == ("geometric_median", 4, False, False)
    net.pool.iterations = 2
    assert net._hip_head() == ("geometric_median", 2, False, False)     # the iteration count is part of the device net's key
    full = cirnet.init_cirnet(pooling=dict(given), **dict(BASE, local_whitening=True, whitening=True))
    assert full._hip_head() == ("geometric_median", 4, True, True) and len(full.parameter_groups({"lr": 1.0})) == 4
    att = cirnet.init_cirnet_attention({"type": "l2norm", "normalize_max": True}, pooling=dict(given), **BASE)
    assert type(att) is cirnet.CirRetrievalNetAttention and type(att.pool) is GM and att._hip_head() == ("geometric_median", 4, False, False)
    assert att._hip_variant() == (("attention", ("l2norm", True)),)
    inchan = cirnet.init_cirnet_inchan({"channels": 1, "preprocessing": {"type": "edgefilter"}}, pooling=dict(given), **BASE)
    assert type(inchan) is cirnet.CirRetrievalNetPreprocessing and type(inchan.pool) is GM and inchan.meta["in_channels"] == 1
    from gandtr_amd.components.model import network as registry
    reg = registry.initialize_model(dict(BASE, architecture="cirnet", pooling=dict(given)))
    assert type(reg.pool) is GM and reg.meta["pooling"] == kept


def test_refusals():
    gm = {"type": "GeometricMedianWeiszfeld", "iterations": 3, "intermediate_gradients": False}
    for bad in ({"type": "HordeCascadedKOrder", "dim": 512, "order": 2, "high_order_dims": 64}, {"type": "gem"}, {"type": "nosuch"}, {"iterations": 3}):
        with pytest.raises(NotImplementedError, match="dict"):
            cirnet.init_cirnet(pooling=bad, **BASE)
    with pytest.raises(NotImplementedError, match="list"):           # the reason Horde stays refused
        cirnet.init_cirnet(pooling={"type": "HordeCascadedKOrder"}, **BASE)
    with pytest.raises(NotImplementedError, match="regional"):
        cirnet.init_cirnet(pooling=dict(gm), **dict(BASE, regional=True))
    with pytest.raises(TypeError):                                    # as the reference's constructor
        cirnet.init_cirnet(pooling={"type": "GeometricMedianWeiszfeld", "intermediate_gradients": False}, **BASE)
    with pytest.raises(TypeError):
        cirnet.init_cirnet(pooling=dict(gm, nosuch=1), **BASE)
    for kw in (dict(whitening=True), dict(local_whitening=True)):     # the attention net takes no whitening, with this pooling either
        with pytest.raises((AssertionError, NotImplementedError)):
            cirnet.init_cirnet_attention({"type": "l2norm", "normalize_max": True}, pooling=dict(gm), **dict(BASE, **kw))
    net = cirnet.init_cirnet(pooling=dict(gm), **BASE)
    for iterations in (-1, 65, 2.5):
        net.pool.iterations = iterations
        with pytest.raises(NotImplementedError, match="iterations"):
            net._hip_head()
    with pytest.raises(ValueError):
        engine.geometric_median(torch.zeros((1, 4, 4, 64)), 3)         # not on a device


@pytest.mark.parametrize("case", M.NET_CASES, ids=M.case_name)
def test_nets_equal_the_reference(golden, case):
    name = M.case_name(case)
    net = M.build_net(INITS, case, int(golden["net_%s_seed" % name]))
    keys, sums = M.head_sums(net)
    assert keys == [str(k) for k in golden["net_%s_keys" % name]]
    assert np.allclose(sums, golden["net_%s_sums" % name], rtol=0, atol=1e-9)
    with torch.no_grad():
        out = net(M.case_input(case)).numpy()                        # the whole batch at once: the mirror treats every image on its own
    ref = golden["net_%s_out" % name]
    assert out.shape == ref.shape == (net.meta["outputdim"], 2)
    assert np.abs(out - ref).max() <= 2e-6, np.abs(out - ref).max()   # (the slack test_attention_host.py allows another host's oneDNN)


def test_checkpoint_round_trip(tmp_path):
    """a checkpoint stores the model's params, the dict with its type among them; Checkpoints.load_network + initialize_network rebuild the pooling"""
    from gandtr_amd.learning import network as netmod
    from gandtr_amd.learning.checkpoints import Checkpoints
    model = dict(BASE, architecture="cirnet", whitening=True, pooling={"type": "GeometricMedianWeiszfeld", "iterations": 2, "intermediate_gradients": False})
    params = {"type": "SingleNetwork", "model": model, "initialize": False,
              "runtime": {"data": {"transforms": "pil2np | totensor"}, "wrappers": "cirfaketuplebatch"}}
    runtime = dict(params["runtime"])
    torch.manual_seed(3)
    net = netmod.initialize_network(params, "cpu").eval()
    path = str(tmp_path / "ck.pth")
    torch.save(net.state_dict()["net"], path)
    again = netmod.initialize_network(None, "cpu", Checkpoints.load_network(path), runtime).eval()
    assert type(again.model) is type(net.model) and again.model.meta == net.model.meta
    assert type(again.model.pool) is GM and again.model.pool.iterations == 2 and again.model.meta["pooling"]["type"] == "GeometricMedianWeiszfeld"
    x = synth.synth_input(7, (2, 3, 64, 96))
    with torch.no_grad():
        assert torch.equal(net(x), again(x))


# ---------------------------------------------------------------------------------------------------------------- C ABI and planner (host code)
def host_graph():
    """a layer graph without a device: the builder calls and the planner are host code"""
    net = engine.HipNet.__new__(engine.HipNet)
    net.lib, net.precision, net.handle = _hip.load(), "f16", ctypes.c_void_p()
    net._group_factor, net._geo_cache, net._finalized = 1.0, {}, False
    _hip.check(net.lib.gdt_net_create(ctypes.byref(net.handle)))
    return net


GEOMETRIES = ((1, 512, 512), (32, 1024, 1024), (3, 160, 1152))


@pytest.mark.parametrize("iterations", [0, 3, 10])
def test_plan_counts(iterations):
    """the planner's count (host logic, no GPU): the map is read iterations + 1 times, in a number of launches that depends on neither batch nor map size"""
    sd = synth.vgg16_state(0)
    sd["whiten.weight"], sd["whiten.bias"] = torch.eye(512), torch.zeros(512)
    for whiten in (False, True):
        net = host_graph()
        f = engine._vgg16_trunk(net, net.input(3), sd)
        net.median_head(f, iterations, whiten=(sd["whiten.weight"], sd["whiten.bias"]) if whiten else None)
        counts = [net.head_launches(*g) for g in GEOMETRIES]
        assert [c[1] for c in counts] == [iterations + 1] * 3
        assert len({c[0] for c in counts}) == 1 and counts[0][0] == 2 * (iterations + 1) + 1 + (2 if whiten else 0)
        assert {net.attention_launches(*g) for g in GEOMETRIES} == {(0, 0)}
        assert net.output_shapes(3, 160, 224) == [(3, 512)] and net.workspace_bytes(3, 160, 224) > 0
    for nmax in (False, True):
        net = host_graph()
        f = engine._vgg16_trunk(net, net.input(3), sd)
        net.median_head(f, iterations, attention=("l2norm", nmax))
        assert {net.head_launches(*g) for g in GEOMETRIES} == {(2 * (iterations + 1) + 1, iterations + 1)}
        assert {net.attention_launches(*g) for g in GEOMETRIES} == {(2 if nmax else 1, iterations + 2)}


def test_a_median_head_changes_no_other_plan():
    """the pool head's and the plain GeM embedder's counts, as tests/test_attention_host.py pins them"""
    sd = synth.vgg16_state(0)
    net = host_graph()
    net.pool_head(engine._vgg16_trunk(net, net.input(3), sd), "mac", aggregate=1)
    assert net.head_launches(2, 512, 512) == (3, 1) and net.attention_launches(2, 512, 512) == (0, 0)
    net = host_graph()
    net.gem_l2n(engine._vgg16_trunk(net, net.input(3), sd), 3.0)
    assert net.head_launches(2, 512, 512) == (0, 0) and net.workspace_bytes(1, 512, 512) == 46137600


def test_argument_errors_without_a_gpu():
    """argument validation happens before any HIP call"""
    lib = _hip.load()
    need = ctypes.c_size_t()
    for args in ((0, 4, 4, 64), (1, 0, 4, 64), (1, 4, 4, 32), (1, 4, 4, 96), (1, 4, 4, 4160), (1, 40000, 4, 64)):
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_geometric_median_workspace_bytes(*args, ctypes.byref(need)))
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_geometric_median_workspace_bytes(1, 4, 4, 64, None))
    _hip.check(lib.gdt_geometric_median_workspace_bytes(2, 32, 32, 512, ctypes.byref(need)))
    assert need.value == 4 * (2 * 32 * 512 + 2 * 32 + 2 * 512)        # 32 workgroups per image: their sums, their weights, the previous median
    _hip.check(lib.gdt_geometric_median_workspace_bytes(2, 1, 3, 64, ctypes.byref(need)))
    assert need.value == 4 * (2 * 64 + 2 + 2 * 64)
    fake = ctypes.c_void_p(4096)                                       # never dereferenced: every call below is refused before any HIP call
    ok = dict(fmap=fake, f32=0, n=1, h=4, w=4, d=64, iterations=3, scale=None, prior=None, out=fake, ws=fake, ws_bytes=1 << 20, stream=None)
    for change in (dict(fmap=None), dict(out=None), dict(f32=2), dict(d=32), dict(d=96), dict(iterations=-1), dict(iterations=65), dict(ws=None),
                   dict(ws_bytes=16), dict(n=0), dict(h=0)):
        a = dict(ok, **change)
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_geometric_median(a["fmap"], a["f32"], a["n"], a["h"], a["w"], a["d"], a["iterations"], a["scale"], a["prior"], a["out"],
                                                a["ws"], a["ws_bytes"], a["stream"]))
    net = host_graph()
    x = net.input(3)
    sd = synth.vgg16_state(0)
    f = net.conv(x, sd["features.0.weight"], sd["features.0.bias"], pad=1, relu=True)
    out = ctypes.c_int()
    eye = np.eye(64, dtype=np.float32)
    peye = eye.ctypes.data_as(ctypes.c_void_p)
    for t, args in ((f, (-1, None, None, 1e-6, 0, 0)),                # iterations
                    (f, (65, None, None, 1e-6, 0, 0)),
                    (f, (3, None, None, 1e-6, 2, 0)),                 # unknown attention
                    (f, (3, None, None, 1e-6, 1, 2)),                 # normalize_max
                    (f, (3, peye, peye, 1e-6, 1, 0)),                 # attention with a final whitening
                    (f, (3, peye, None, 1e-6, 0, 0)),                 # a weight without its bias
                    (x, (3, None, None, 1e-6, 0, 0)),                 # channels % 64
                    (99, (3, None, None, 1e-6, 0, 0))):               # tensor id
        ops = lib.gdt_net_num_ops(net.handle)
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_net_median_head(net.handle, t, ctypes.byref(_hip.MedianHeadDesc(*args)), ctypes.byref(out)))
        assert lib.gdt_net_num_ops(net.handle) == ops                  # a refused head leaves nothing in the graph
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_net_median_head(net.handle, f, None, ctypes.byref(out)))
    with pytest.raises(NotImplementedError):
        net.median_head(f, 3, attention=("nosuch", False))
    assert net.median_head(f, 3) >= 0
