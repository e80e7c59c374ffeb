"""The descriptor heads on the host (no GPU): the C region grid and the torch mirror of cirtorch's pooling layers / init_network against what the
reference itself produced (tests/golden/descriptor_heads.npz, written by tests/golden/make_descriptor_heads_golden.py)."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_descriptor_heads_golden as G                        # noqa: E402  (seeded inputs, case lists; imports no reference code)
from gandtr_amd import _hip                                     # noqa: E402
from gandtr_amd.components.model.network import cirnet          # noqa: E402
from gandtr_amd.tools import synth                              # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "descriptor_heads.npz"))


def c_regions(h, w, levels):
    lib = _hip.load()
    n = ctypes.c_int()
    _hip.check(lib.gdt_rpool_regions(h, w, levels, None, 0, ctypes.byref(n)))
    buf = (ctypes.c_int * (4 * n.value))()
    _hip.check(lib.gdt_rpool_regions(h, w, levels, buf, n.value, ctypes.byref(n)))
    return np.array(list(buf), dtype=np.int64).reshape(n.value, 4)


def mirror_regions(h, w, levels):
    return np.array([(0, 0, h, w)] + [(y, x, s, s) for y, x, s in cirnet.region_grid(h, w, levels)], dtype=np.int64)


def test_region_grid_equals_the_reference_for_every_size(golden):
    """gdt_rpool_regions (C, what the planner uses) and cirnet.region_grid (torch, what the CPU path uses) for all 5184 sizes at L = 3"""
    counts, boxes = golden["grid_counts"], golden["grid_boxes"].astype(np.int64)
    assert counts.shape == (G.GRID_MAX, G.GRID_MAX) and counts.min() == 2 and counts.max() == 51
    off, bad = 0, []
    for h in range(1, G.GRID_MAX + 1):
        for w in range(1, G.GRID_MAX + 1):
            n = int(counts[h - 1, w - 1])
            ref = boxes[off:off + n]
            off += n
            if not np.array_equal(c_regions(h, w, 3), ref):
                bad.append(("C", h, w))
            if not np.array_equal(mirror_regions(h, w, 3), ref):
                bad.append(("mirror", h, w))
    assert off == len(boxes)
    assert not bad, bad[:20]


def test_region_grid_other_level_counts(golden):
    for k, (L, h, w) in enumerate(golden["grid_extra"].tolist()):
        ref = golden["grid_extra_%d" % k].astype(np.int64)
        assert np.array_equal(c_regions(h, w, L), ref), (L, h, w)
        assert np.array_equal(mirror_regions(h, w, L), ref), (L, h, w)
    assert len(c_regions(9, 9, 0)) == 1


def test_region_grid_bad_arguments():
    lib = _hip.load()
    n = ctypes.c_int()
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_rpool_regions(0, 5, 3, None, 0, ctypes.byref(n)))
    buf = (ctypes.c_int * 8)()
    with pytest.raises(ValueError, match="capacity"):
        _hip.check(lib.gdt_rpool_regions(32, 32, 3, buf, 2, ctypes.byref(n)))
    assert n.value == 15                                        # a square map: 1 + 1 + 4 + 9


def mirror_pools():
    p_mp, rw, rb = G.layer_params()
    lin = torch.nn.Linear(G.LAYER_D, G.LAYER_D)
    lin.load_state_dict({"weight": rw, "bias": rb})
    gemmp = cirnet.GeMmp(mp=G.LAYER_D)
    gemmp.p.data.copy_(p_mp)
    return {"mac": cirnet.MAC(), "spoc": cirnet.SPoC(), "gem3": cirnet.GeM(p=3), "gem237": cirnet.GeM(p=2.37), "gemmp": gemmp,
            "rmac": cirnet.RMAC()}, lin


@pytest.mark.parametrize("si", range(len(G.LAYER_SIZES)))
def test_pooling_layers_equal_the_reference(golden, si):
    pools, lin = mirror_pools()
    with torch.no_grad():
        for kind in G.LAYER_KINDS:
            x = G.layer_map(si, kind)
            for name in G.POOLS:
                ref = golden["layer_%d_%s_%s" % (si, kind, name)]
                got = pools[name](x).numpy()
                assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-6, (kind, name, np.abs(got - ref).max())
            for name in G.RPOOLS:
                for tag, layer in (("r", cirnet.Rpool(pools[name])), ("rw", cirnet.Rpool(pools[name], lin))):
                    ref = golden["layer_%d_%s_%s_%s" % (si, kind, tag, name)]
                    got = layer(x).numpy()
                    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-6, (kind, tag, name, np.abs(got - ref).max())


def test_rpool_without_aggregation():
    x = G.layer_map(1, "relu")
    o = cirnet.Rpool(cirnet.GeM())(x, aggregate=False)
    assert o.shape == (2, len(cirnet.region_grid(32, 21)) + 1, G.LAYER_D, 1, 1)
    assert torch.allclose(o.flatten(2).norm(dim=2), torch.ones(2, o.shape[1]), atol=1e-5)


def test_layer_reprs():
    assert repr(cirnet.MAC()) == "MAC()" and repr(cirnet.SPoC()) == "SPoC()" and repr(cirnet.RMAC()) == "RMAC(L=3)"
    assert repr(cirnet.GeMmp(mp=7)) == "GeMmp(p=[7], eps=1e-06)"
    assert repr(cirnet.Rpool(cirnet.MAC())).endswith("(L=3)")


@pytest.mark.parametrize("case", G.NET_CASES, ids=G.case_name)
def test_nets_equal_the_reference(golden, case):
    """seeded construction draws the reference's numbers (the head layers are created in its order) and the forward gives its descriptors"""
    name = G.case_name(case)
    net = G.build_net(cirnet.init_cirnet, case, int(golden["net_%s_seed" % name]))
    keys, sums = G.head_sums(net)
    assert keys == [str(k) for k in golden["net_%s_keys" % name]]
    assert np.allclose(sums, golden["net_%s_sums" % name], rtol=0, atol=1e-9), (sums, golden["net_%s_sums" % name])
    with torch.no_grad():
        out = net(G.net_input()).numpy()
    ref = golden["net_%s_out" % name]
    assert out.shape == ref.shape == (net.meta["outputdim"], G.NET_INPUT[0])
    assert np.abs(out - ref).max() <= 2e-6, np.abs(out - ref).max()        # (the slack test_oracle_golden.py allows another host's oneDNN)


def _init(**kw):
    params = dict(cir_architecture="vgg16", local_whitening=False, pooling="gem", regional=False, whitening=False, pretrained=False)
    params.update(kw)
    return cirnet.init_cirnet(**params)


def test_state_dict_keys_and_parameter_groups():
    net = _init(local_whitening=True, pooling="gemmp", regional=True, whitening=True)
    head = [k for k in net.state_dict() if not k.startswith("features.")]
    assert head == ["lwhiten.weight", "lwhiten.bias", "pool.rpool.p", "pool.whiten.weight", "pool.whiten.bias", "whiten.weight", "whiten.bias"]
    assert net.state_dict()["pool.rpool.p"].shape == (512,)
    groups = net.parameter_groups({"lr": 0.5})
    ids = lambda ps: [id(p) for p in ps]
    assert [ids(g["params"]) for g in groups] == [ids(net.features.parameters()), ids(net.lwhiten.parameters()), ids(net.pool.rpool.parameters()),
                                                  ids(net.pool.whiten.parameters()), ids(net.whiten.parameters())]
    assert groups[2]["lr"] == 5.0 and groups[2]["weight_decay"] == 0 and all("lr" not in groups[i] for i in (0, 1, 3, 4))
    plain = _init()
    assert [k for k in plain.state_dict() if not k.startswith("features.")] == ["pool.p"] and plain.state_dict()["pool.p"].shape == (1,)
    groups = plain.parameter_groups({"lr": 0.5})
    assert len(groups) == 2 and groups[1]["lr"] == 5.0 and groups[1]["weight_decay"] == 0
    groups = _init(pooling="mac", whitening=True).parameter_groups({"lr": 1.0})
    assert len(groups) == 3 and list(groups[1]["params"]) == []
    assert "whitening: True" in repr(_init(whitening=True))


def test_whitening_from_a_learned_file(tmp_path):
    lw = synth.whitening_state(5, 512)
    path = str(tmp_path / "lw.pkl")
    with open(path, "wb") as f:
        pickle.dump(lw, f)
    net = _init(whitening=path)
    P, m = torch.tensor(lw["P"]), torch.tensor(lw["m"])
    assert torch.equal(net.whiten.weight.data, P) and torch.equal(net.whiten.bias.data, -torch.mm(P, m).squeeze())
    assert net.meta["whitening"] == path

    class Evil:
        def __reduce__(self):
            return (os.getcwd, ())
    with open(path, "wb") as f:
        pickle.dump({"P": Evil()}, f)
    with pytest.raises(pickle.UnpicklingError):
        _init(whitening=path)


def test_refusals_that_remain():
    with pytest.raises(ValueError, match="download"):
        _init(pretrained=True)
    with pytest.raises(NotImplementedError, match="dict"):
        _init(pooling={"type": "gem"})
    with pytest.raises(NotImplementedError, match="R-MAC regions"):
        _init(pooling="rmac", regional=True)
    with pytest.raises(KeyError):
        _init(pooling="nosuch")
    with pytest.raises(ValueError):
        cirnet.init_cirnet(cir_architecture="vgg16", pooling="gem")


def test_checkpoint_with_whitening_round_trips(tmp_path):
    """a checkpoint stores the head in its meta; Checkpoints.load_network rebuilds the model from it"""
    from gandtr_amd.learning import network as netmod
    from gandtr_amd.learning.checkpoints import Checkpoints
    params = {"type": "SingleNetwork",
              "model": {"architecture": "cirnet", "cir_architecture": "vgg16", "local_whitening": False, "pooling": "gem", "pretrained": False,
                        "regional": True, "whitening": True},
              "initialize": False,
              "runtime": {"data": {"transforms": "pil2np | totensor | normalize", "mean_std": [[0.485, 0.456, 0.406], [0.229, 0.224, 0.225]]},
                          "wrappers": "cirfaketuplebatch"}}
    runtime = dict(params["runtime"])
    torch.manual_seed(3)
    net = netmod.initialize_network(params, "cpu").eval()
    path = str(tmp_path / "ck.pth")
    torch.save(net.state_dict()["net"], path)
    state = Checkpoints.load_network(path)
    again = netmod.initialize_network(None, "cpu", state, runtime).eval()
    assert isinstance(again.model.pool, cirnet.Rpool) and again.model.whiten is not None and again.model.meta["whitening"] is True
    x = synth.synth_input(7, (1, 3, 64, 96))
    with torch.no_grad():
        assert torch.equal(net(x), again(x))
