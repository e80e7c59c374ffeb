"""The attention and edge-map variants of the retrieval embedder on the host (no GPU): registries, the torch mirror of the reference's L2NormAttention,
EdgeFilter, init_cirnet_attention and init_cirnet_inchan against what the reference itself produced (tests/golden/attention.npz, written by
tests/golden/make_attention_golden.py), and the planner's counts for the attention head."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_attention_golden as A                               # noqa: E402  (seeded inputs, case lists; imports no reference code)
import make_descriptor_heads_golden as H                        # noqa: E402
from gandtr_amd import _hip, engine                             # noqa: E402
from gandtr_amd.components.model import layers                  # noqa: E402
from gandtr_amd.components.model.network import cirnet, single_layer      # noqa: E402
from gandtr_amd.tools import synth                              # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "attention.npz"))


BASE = dict(cir_architecture="vgg16", local_whitening=False, pooling="gem", regional=False, whitening=False, pretrained=False)


def test_registry_and_alias_identities():
    import mdir                                                  # noqa: F401
    from gandtr_amd.components.model import network as registry
    from mdir.components.model import layers as alias_layers
    from mdir.components.model.layers import attention as alias_attention, preprocessing as alias_preprocessing
    from mdir.components.model.network import MODEL_LABELS, single_layer as alias_single
    assert MODEL_LABELS is registry.MODEL_LABELS
    assert MODEL_LABELS["cirnet_attention"] is cirnet.init_cirnet_attention and MODEL_LABELS["cirnet_inchan"] is cirnet.init_cirnet_inchan
    assert MODEL_LABELS["normalization_l2"] is single_layer.NormalizationL2 is alias_single.NormalizationL2
    assert alias_layers is layers and alias_attention is layers.attention and alias_preprocessing is layers.preprocessing
    assert layers.attention.ATTENTIONS == {"l2norm": layers.attention.L2NormAttention}
    net = registry.initialize_model(dict(BASE, architecture="cirnet_attention", attention={"type": "l2norm", "normalize_max": True}))
    assert isinstance(net, cirnet.CirRetrievalNetAttention) and net.attention.normalize_max is True
    net = registry.initialize_model(dict(BASE, architecture="cirnet_inchan", inputs={"channels": 1, "preprocessing": {"type": "edgefilter", "w": 3}}))
    assert isinstance(net, cirnet.CirRetrievalNetPreprocessing) and net.preprocessing.w == 3.0
    assert net.meta["in_channels"] == 1 and net.meta["preprocessing"] == "edgefilter" and net.features[0].weight.shape[1] == 1
    plain = registry.initialize_model(dict(BASE, architecture="cirnet_inchan", inputs={"channels": 3, "preprocessing": None}))
    assert type(plain) is cirnet.CirRetrievalNet and plain.meta["in_channels"] == 3 and "preprocessing" not in plain.meta


def test_normalization_l2():
    layer = single_layer.NormalizationL2()
    assert layer.meta == {}
    x = synth.synth_input(9, (3, 16))
    assert torch.equal(layer(x), x / (torch.norm(x, p=2, dim=1, keepdim=True) + 1e-6))


@pytest.mark.parametrize("si", A.ATT_SIZES)
def test_attention_layer_equals_the_reference(golden, si):
    for kind in H.LAYER_KINDS:
        x = H.layer_map(si, kind)
        for nmax in (False, True):
            layer = layers.attention.L2NormAttention(nmax)
            got = torch.stack([layer(x[i:i + 1]).reshape(x.shape[2:]) for i in range(x.size(0))]).numpy()
            ref = golden["att_%d_%s_%d" % (si, kind, nmax)]
            assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-6 * max(1.0, ref.max()), (kind, nmax, np.abs(got - ref).max())
            if nmax:
                assert (got.reshape(got.shape[0], -1).max(axis=1) == 1.0).all()


@pytest.mark.parametrize("k", range(len(A.FILTER_SETS)))
def test_edge_filter_equals_the_reference_and_writes_the_clamp_back(golden, k):
    layer = layers.preprocessing.EdgeFilter(**A.FILTER_SETS[k])
    params = A.filter_params(k)
    assert layer.tau.item() == np.float32(params["tau"]) and layer.w == params["w"] and layer.beta == params["beta"] and layer.eps == params["eps"]
    assert list(layer.state_dict()) == ["p", "tau"]
    x = A.filter_input()
    assert (x == 0).sum() > 100 and ((x - 0.1).abs() < 1e-3).sum() > 100 and ((x - 0.9).abs() < 1e-3).sum() > 100       # the fixture's input is what it says
    with torch.no_grad():
        got = layer(x).numpy()
    ref = golden["filter_%d_out" % k]
    assert np.abs(got - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max()), np.abs(got - ref).max()
    assert torch.equal(layer.tau.data, torch.from_numpy(golden["filter_%d_tau" % k]))
    assert layer.tau.item() == np.float32(min(max(params["tau"], 0.01), 0.9))
    low = layers.preprocessing.EdgeFilter(tau=-3.0)
    low(x)
    assert low.tau.item() == np.float32(0.01)
    assert repr(layers.preprocessing.EdgeFilter()) == "EdgeFilter(w=10.0000, p=0.5000, beta=500.0000, tau=0.1000, eps=0.000001)"


def _check_net(golden, name, net, x):
    keys, sums = A.head_sums(net)
    assert keys == [str(k) for k in golden["net_%s_keys" % name]]
    assert np.allclose(sums, golden["net_%s_sums" % name], rtol=0, atol=1e-9), (sums, golden["net_%s_sums" % name])
    with torch.no_grad():
        out = net(x).numpy()                                         # the whole batch at once: the mirror treats every image on its own
    ref = golden["net_%s_out" % name]
    assert out.shape == ref.shape == (net.meta["outputdim"], 2)
    assert np.abs(out - ref).max() <= 2e-6, np.abs(out - ref).max()   # (the slack test_oracle_golden.py allows another host's oneDNN)


@pytest.mark.parametrize("case", A.ATT_CASES, ids=A.att_name)
def test_attention_nets_equal_the_reference(golden, case):
    name = A.att_name(case)
    _check_net(golden, name, A.build_att_net(cirnet.init_cirnet_attention, case, int(golden["net_%s_seed" % name])), A.att_input())


@pytest.mark.parametrize("case", A.INCHAN_CASES, ids=A.inchan_name)
def test_inchan_nets_equal_the_reference(golden, case):
    name = A.inchan_name(case)
    _check_net(golden, name, A.build_inchan_net(cirnet.init_cirnet_inchan, case, int(golden["net_%s_seed" % name])), A.net_input(case[1]))


def test_a_batch_equals_its_images_one_by_one():
    """the head on a given map: bit for bit (per-image attention, per-image maximum); the whole net: to the rounding of a conv that sees another batch size"""
    fmap = torch.relu(synth.synth_input(11, (3, 512, 9, 13)))
    fmap[1] *= 7.0                                                   # images of different maxima
    for case in (("vgg16", "gem", False, True), ("vgg16", "rmac", False, True), ("vgg16", "gem", True, False)):
        net = A.build_att_net(cirnet.init_cirnet_attention, case, 1000)
        with torch.no_grad():
            whole = net._head(fmap)
            single = torch.cat([net._head(fmap[i:i + 1]) for i in range(3)], dim=1)
        assert torch.equal(whole, single), case
    net = A.build_att_net(cirnet.init_cirnet_attention, ("vgg16", "gem", False, True), 1000)
    x = synth.synth_input(12, (2, 3, 64, 96))
    with torch.no_grad():
        assert (net(x) - torch.cat([net(x[:1]), net(x[1:])], dim=1)).abs().max() <= 2e-6


def test_parameter_groups():
    ids = lambda ps: [id(p) for p in ps]
    net = cirnet.init_cirnet_attention({"type": "l2norm", "normalize_max": False}, **dict(BASE, regional=True))
    groups = net.parameter_groups({"lr": 0.5})
    assert [ids(g["params"]) for g in groups] == [ids(net.features.parameters()), ids(net.pool.rpool.parameters()), ids(net.pool.whiten.parameters()), []]
    assert groups[1]["lr"] == 5.0 and groups[1]["weight_decay"] == 0 and groups[3]["lr"] == 50.0 and "weight_decay" not in groups[3]
    assert "lr" not in groups[0] and "lr" not in groups[2]
    net = cirnet.init_cirnet_inchan({"channels": 1, "preprocessing": {"type": "edgefilter"}}, **BASE)
    groups = net.parameter_groups({"lr": 0.5})
    assert [ids(g["params"]) for g in groups] == [ids(net.features.parameters()), ids(net.pool.parameters()), ids([net.preprocessing.p, net.preprocessing.tau])]
    assert groups[1]["lr"] == 5.0 and groups[1]["weight_decay"] == 0 and groups[2]["lr"] == 5.0 and "weight_decay" not in groups[2]
    assert [k for k in net.state_dict() if not k.startswith("features.")] == ["pool.p", "preprocessing.p", "preprocessing.tau"]


def test_refusals():
    for kw in (dict(whitening=True), dict(local_whitening=True)):
        with pytest.raises((AssertionError, NotImplementedError)):
            cirnet.init_cirnet_attention({"type": "l2norm", "normalize_max": True}, **dict(BASE, **kw))
    with pytest.raises(KeyError):
        cirnet.init_cirnet_attention({"type": "nosuch"}, **BASE)
    with pytest.raises(NotImplementedError, match="channels"):
        cirnet.init_cirnet_inchan({"channels": 2, "preprocessing": None}, **BASE)
    with pytest.raises(NotImplementedError, match="preprocessing"):
        cirnet.init_cirnet_inchan({"channels": 1, "preprocessing": {"type": "nosuch"}}, **BASE)


@pytest.mark.parametrize("model", [
    dict(BASE, architecture="cirnet_attention", attention={"type": "l2norm", "normalize_max": True}, regional=True),
    dict(BASE, architecture="cirnet_inchan", inputs={"channels": 1, "preprocessing": {"type": "edgefilter", "tau": 0.3, "p": 0.7}})],
    ids=["attention", "inchan"])
def test_checkpoint_round_trips(tmp_path, model):
    """a checkpoint stores the model's params; Checkpoints.load_network + initialize_network rebuild the variant, its layer settings and its channel count"""
    from gandtr_amd.learning import network as netmod
    from gandtr_amd.learning.checkpoints import Checkpoints
    params = {"type": "SingleNetwork", "model": model, "initialize": False,
              "runtime": {"data": {"transforms": "pil2np | totensor"}, "wrappers": "cirfaketuplebatch"}}
    runtime = dict(params["runtime"])
    torch.manual_seed(3)
    net = netmod.initialize_network(params, "cpu").eval()
    if model["architecture"] == "cirnet_inchan":
        with torch.no_grad():
            net.model.preprocessing.tau.fill_(0.45)                   # a trained value: it has to come back from the state, not from the params
    path = str(tmp_path / "ck.pth")
    torch.save(net.state_dict()["net"], path)
    again = netmod.initialize_network(None, "cpu", Checkpoints.load_network(path), runtime).eval()
    assert type(again.model) is type(net.model) and again.model.meta == net.model.meta
    if model["architecture"] == "cirnet_attention":
        assert again.model.attention.normalize_max is True and isinstance(again.model.pool, cirnet.Rpool)
        x = synth.synth_input(7, (1, 3, 64, 96))
    else:
        assert again.model.preprocessing.tau.item() == np.float32(0.45) and again.model.preprocessing.p.item() == np.float32(0.7)
        assert again.model.features[0].weight.shape[1] == 1 and again.model.meta["in_channels"] == 1
        x = A.net_input(1)[:1, :, :64, :96]
    with torch.no_grad():
        assert torch.equal(net(x), again(x))


def host_graph():
    """a layer graph without a device: the builder calls and the planner are host code"""
    net = engine.HipNet.__new__(engine.HipNet)
    net.lib, net.precision, net.handle = _hip.load(), "f16", ctypes.c_void_p()
    net._group_factor, net._geo_cache, net._finalized = 1.0, {}, False
    _hip.check(net.lib.gdt_net_create(ctypes.byref(net.handle)))
    return net


GEOMETRIES = ((1, 512, 512), (8, 512, 512), (32, 1024, 1024), (2, 1024, 352), (3, 160, 1152))


def test_attention_launches_do_not_depend_on_batch_or_regions():
    """the planner's count (host logic, no GPU): the attention adds the norm pass (+ the division by the maximum); the head reads the map twice"""
    sd = synth.vgg16_state(0)
    sd["pool.whiten.weight"], sd["pool.whiten.bias"] = torch.eye(512), torch.zeros(512)
    for kind, aggregate, rwhiten, head in (("gem", 0, False, 2), ("mac", 1, False, 3), ("gem", 2, True, 6), ("spoc", 2, False, 4)):
        for nmax in (False, True):
            net = host_graph()
            f = engine._vgg16_trunk(net, net.input(3), sd)
            net.pool_head_attention(f, kind, nmax, p=sd["pool.p"] if kind == "gem" else None, aggregate=aggregate,
                                    rwhiten=(sd["pool.whiten.weight"], sd["pool.whiten.bias"]) if rwhiten else None)
            assert {net.attention_launches(*g) for g in GEOMETRIES} == {(2 if nmax else 1, 2)}, (kind, aggregate, nmax)
            assert {net.head_launches(*g) for g in GEOMETRIES} == {(head, 1)}, (kind, aggregate, nmax)
            assert net.output_shapes(3, 160, 224) == [(3, 512)]


def test_other_embedders_count_no_attention_and_plan_as_before():
    sd = synth.vgg16_state(0)
    for with_head in (False, True):
        net = host_graph()
        f = engine._vgg16_trunk(net, net.input(3), sd)
        if with_head:
            net.pool_head(f, "mac", aggregate=1)
        else:
            net.gem_l2n(f, 3.0)
        assert net.attention_launches(2, 512, 512) == (0, 0) and net.head_launches(2, 512, 512) == ((3, 1) if with_head else (0, 0))
        if not with_head:                                            # the figures tests/test_hip_descriptor_heads.py pins for the plain GeM embedder
            plan = net.plan_summary(1, 512, 512)
            pinned = dict(conv_launches=13, bottlenecks_fused=0, conv3x3_expand=0, chained_reduce=0, shortcuts_folded=0, norms_folded=0, pools_fused=4,
                          direct_stem=1, transposed_fused=0, stride2_shift=0, dilated_convs=0, dilated_special_forms=0)
            assert {k: plan[k] for k in pinned} == pinned
            assert all(v == 0 for k, v in plan.items() if k not in pinned), plan            # every other counter
            assert net.workspace_bytes(1, 512, 512) == 46137600


def test_filtered_and_one_channel_inputs_are_packed():
    """the stem forms that read the caller's image are not planned for an input with a filter or without three channels"""
    sd = synth.vgg16_state(0)
    sd1 = dict(sd)
    sd1["features.0.weight"] = sd["features.0.weight"].sum(dim=1, keepdim=True)
    for channels, filt, direct in ((3, False, 1), (3, True, 0), (1, False, 0), (1, True, 0)):
        for precision in (0, 1):
            net = host_graph()
            _hip.check(net.lib.gdt_net_set_precision(net.handle, precision))
            x = net.input(channels)
            if filt:
                net.input_filter("edgefilter", 10, 0.5, 500, 0.1, 1e-6)
            engine._vgg16_trunk(net, x, sd if channels == 3 else sd1)
            assert net.plan_summary(32, 1024, 1024)["direct_stem"] == (direct if precision == 0 else 0), (channels, filt, precision)
            net.output_shapes(2, 160, 224)


def test_builder_argument_validation():
    net = host_graph()
    with pytest.raises(ValueError):
        net.input_filter("edgefilter", 10, 0.5, 500, 0.1, 1e-6)        # no input yet
    x = net.input(1)
    with pytest.raises(ValueError):
        net.input_filter("edgefilter", 10, 0.5, 500, 0.1, 0.0)         # eps
    with pytest.raises(ValueError):
        net.input_filter("edgefilter", float("nan"), 0.5, 500, 0.1, 1e-6)
    with pytest.raises(NotImplementedError):
        net.input_filter("nosuch", 10, 0.5, 500, 0.1, 1e-6)
    net.input_filter("edgefilter", 10, 0.5, 500, 0.1, 1e-6)
    with pytest.raises(ValueError):
        net.input_filter("edgefilter", 10, 0.5, 500, 0.1, 1e-6)        # once
    sd = synth.vgg16_state(0)
    f = net.conv(x, sd["features.0.weight"].sum(dim=1, keepdim=True), sd["features.0.bias"], pad=1, relu=True)
    lib, out = net.lib, ctypes.c_int()
    one = (ctypes.c_float * 1)(3.0)
    pone = ctypes.cast(one, ctypes.c_void_p)
    for t, args in ((f, (2, pone, 1, 1e-6, 0, 3, None, None, None, None, 1e-6, 2, 0)),       # unknown attention
                    (f, (2, pone, 1, 1e-6, 0, 3, None, None, None, None, 1e-6, 1, 2)),       # normalize_max
                    (f, (2, None, 0, 1e-6, 0, 3, None, None, None, None, 1e-6, 1, 0)),       # GeM without its exponent
                    (99, (0, None, 0, 1e-6, 0, 3, None, None, None, None, 1e-6, 1, 0))):     # tensor id
        ops = lib.gdt_net_num_ops(net.handle)
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_net_pool_head(net.handle, t, ctypes.byref(_hip.PoolHeadDesc(*args)), ctypes.byref(out)))
        assert lib.gdt_net_num_ops(net.handle) == ops                  # a refused head leaves nothing in the graph
    bytes_ = ctypes.c_size_t()
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_pixel_attention_workspace_bytes(0, 4, 4, ctypes.byref(bytes_)))
    _hip.check(lib.gdt_pixel_attention_workspace_bytes(2, 32, 32, ctypes.byref(bytes_)))
    assert bytes_.value == 2 * 64 * 4                                  # one maximum per workgroup of 16 pixels
    for call in (lambda: lib.gdt_pixel_attention(None, 0, 1, 4, 4, 64, 0, None, None, 0, None),
                 lambda: lib.gdt_pool_regions_weighted(None, 0, 1, 4, 4, 64, 0, 3.0, None, 1e-6, 0, None, None, None),
                 lambda: lib.gdt_pack_input_filter(None, 1, 1, 4, 4, 1, 1, 10.0, 0.5, 500.0, 0.1, 1e-6, None, None)):
        with pytest.raises(ValueError):
            _hip.check(call())
