"""The grouping layers on CPU tensors (components/model/layers/grouping.py, functional.py) against tests/golden/grouping.npz, which
tests/golden/make_grouping_golden.py wrote from the reference's layers; their configuration mini-language; codebook loading (no GPU)."""
import os
import pickle

import numpy as np
import pytest
import torch

import codebook_bound as B
import grouping_fixture as G

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grouping.npz"))


def _layers():
    from gandtr_amd.components.model.layers import functional, grouping
    return functional, grouping


def _close(got, ref, label):
    scale = max(float(np.abs(ref).max()), 1e-30)
    err = float(np.abs(got.numpy() - ref).max()) / scale
    print("%s: max |d| / max |ref| = %.2e" % (label, err))
    assert got.shape == ref.shape and err <= 1e-6, (label, err)


@pytest.mark.parametrize("name", list(G.CASES))
def test_cpu_layers_match_the_reference_values(name):
    _, grouping = _layers()
    grouped, weights = G.run(G.build(grouping.GROUPINGS, name), name, G.images())
    _close(grouped, GOLDEN[name + "_grouped"], name + " grouped")
    _close(weights, GOLDEN[name + "_weights"], name + " weights")
    assert not grouped[1].any() and not weights[1].any()                 # the empty image
    assert float(GOLDEN[name + "_gap"]) >= G.GAP


@pytest.mark.parametrize("name", G.HARD)
def test_reference_values_lie_inside_the_float64_bound(name):
    """the bound test_hip_grouping.py holds the device to also holds the reference's own fp32 evaluation"""
    _, features, nearest, assignment, descriptor, weights, _ = G.CASES[name]
    imgs = G.images()
    x = torch.cat([f for fs, _ in imgs for f in fs]).numpy()
    att = torch.cat([a for _, at in imgs for a in at]).numpy()
    kind, *base = assignment.split("-")
    dname, *dparam = descriptor.split("-")
    ma = int(nearest.split("-")[1]) if "-" in nearest else 1
    r = B.grouping_ref(x, att, G.codebook().numpy(), G.SIZES, features, ma, kind, float(base[0]) if base else 0.0, dname,
                       float(dparam[0]) if dparam else 0.0, weights)
    assert B.within(GOLDEN[name + "_grouped"], r["grouped"], r["grouped_b"]) <= 1.0
    assert B.within(GOLDEN[name + "_weights"], r["weights"], r["weights_b"]) <= 1.0


def test_groupings_table_repr_and_mini_language():
    _, grouping = _layers()
    assert list(grouping.GROUPINGS) == ["BatchClustering", "ClusteringCodebook", "LoadedCodebook", "FaissCodebook"]
    layer = G.build(grouping.GROUPINGS, "normresatt")
    assert repr(layer) == "LoadedCodebook(centroids=7, features=normresatt, nearest=top-3, assignment=softmax-2.0, descriptor=l2norm, weights=maxassatt)"
    assert repr(G.build(grouping.GROUPINGS, "batch")) == ("BatchClustering(centroids=5, features=iden, nearest=top, assignment=uniform, descriptor=l2norm, "
                                                          "weights=unif, clustering=kmeans, iterations=2)")
    assert layer.params == {"centroids": 7, "features": "normresatt", "nearest": "top-3", "assignment": "softmax-2.0", "descriptor": "l2norm",
                            "weights": "maxassatt"}
    call = grouping.Grouping.str_func_call
    table = {"f": lambda *a, **k: (a, k)}
    assert call("f-3-2.5-detach", table) == ((3, 2.5), {"detach": True})
    assert call("F", table) == ((), {})
    assert call("top-3", grouping.Grouping.nearest_params) == 3 and call("top", grouping.Grouping.nearest_params) == 1
    assert call("all", grouping.Grouping.nearest_params) is None
    with pytest.raises(KeyError):
        call("nosuch-1", table)
    assert grouping.Grouping._parse_size("64k") == 65536 and grouping.Grouping._parse_size(12) == 12
    assert grouping.SIZE_SHORTCUTS["1k"] == 1024 and grouping.SIZE_SHORTCUTS["512k"] == 524288 and len(grouping.SIZE_SHORTCUTS) == 10
    assert set(grouping.Grouping.feature_functions) == set(B.FEATURES) | {"normressoftmaxatt"}
    with pytest.raises(AssertionError):                                   # top_centroids needs a max / sum / avg / unif weight function
        grouping.LoadedCodebook(G.codebook(), "iden", "top", "uniform", "l2norm", "descnorm3", 1.0, 4, outputdim=G.D)


def test_forward_flattens_maps_like_the_reference():
    _, grouping = _layers()
    layer = G.build(grouping.GROUPINGS, "iden")
    x, a = torch.randn(G.D, 3, 4), torch.rand(3, 4) + 0.1
    with torch.no_grad():
        g1, w1 = layer([([x], [a])])
        g2, w2 = layer._forward([([x.reshape(G.D, -1).T], [a.reshape(-1, 1)])])
    assert torch.equal(g1, g2) and torch.equal(w1, w2) and g1.shape == (1, G.K, G.D)


def test_loaded_codebook_from_pickle_and_foreign_types_are_refused(tmp_path):
    _, grouping = _layers()
    c = G.codebook()
    path = str(tmp_path / "codebook.pkl")
    with open(path, "wb") as handle:
        pickle.dump({"state": {"centroids": c.numpy()}}, handle)
    layer = grouping.LoadedCodebook(path, "iden", "top", "uniform", "l2norm", "unif", 1.0, 0, outputdim=G.D)
    assert torch.equal(layer.codebook.data, c) and isinstance(layer.codebook, torch.nn.Parameter)
    assert grouping.LoadedCodebook.load_codebook(c) is c
    bad = str(tmp_path / "bad.pkl")
    with open(bad, "wb") as handle:
        pickle.dump({"state": {"centroids": c.numpy(), "extra": os.path.join}}, handle)          # a callable from a foreign module
    with pytest.raises(pickle.UnpicklingError):
        grouping.LoadedCodebook.load_codebook(bad)


def test_iterate_kmeans_matches_the_reference_and_keeps_an_emptied_cluster():
    functional, _ = _layers()
    feats = torch.cat([f for fs, _ in G.images() for f in fs])
    out = functional.iterate_kmeans(feats, torch.from_numpy(GOLDEN["kmeans_start"].copy()), 2)
    _close(out, GOLDEN["kmeans_out"], "iterate_kmeans")
    torch.manual_seed(G.BATCH_SEED)
    assert np.array_equal(functional.init_clusters_forgy(feats, 5).numpy(), GOLDEN["kmeans_start"])      # the same seed picks the same points
    start = torch.cat([torch.from_numpy(GOLDEN["kmeans_start"].copy()), torch.full((1, G.D), 100.0)])
    out = functional.iterate_kmeans(feats, start.clone(), 2)
    assert torch.equal(out[5], start[5]) and bool(torch.isfinite(out).all())
    _close(out[:5], GOLDEN["kmeans_out"], "iterate_kmeans beside an empty cluster")


def test_clustering_and_faiss_codebooks():
    functional, grouping = _layers()
    feats = torch.cat([f for fs, _ in G.images() for f in fs])
    layer = grouping.ClusteringCodebook(5, "iden", "top", "uniform", "l2norm", "unif", 1.0, 0, 2, outputdim=G.D)
    assert layer.params["iterations"] == 2 and tuple(layer.codebook.shape) == (5, G.D) and not layer.codebook.any()
    torch.manual_seed(G.BATCH_SEED)
    layer.compute_codebook(feats)
    _close(layer.codebook.data, GOLDEN["kmeans_out"], "ClusteringCodebook.compute_codebook")
    faiss = grouping.FaissCodebook("1k", "iden", "top", "uniform", "l2norm", "unif", 1.0, 0, outputdim=G.D)
    assert tuple(faiss.codebook.shape) == (1024, G.D)
    with pytest.raises(ImportError):
        faiss.compute_codebook(feats)
    w = functional.assign_weights_softmax(torch.tensor([[0.0, 1.0]]), 2.0)
    assert torch.allclose(w, torch.softmax(torch.tensor([[0.0, -2.0]]), dim=1))
    assert torch.equal(functional.idx2rank_dim1(torch.tensor([[2, 0, 1]])), torch.tensor([[1, 2, 0]]))


def test_reference_module_alias_resolves():
    import mdir                                                             # noqa: F401
    from mdir.components.model.layers import functional as f, grouping as g
    from gandtr_amd.components.model.layers import functional, grouping
    assert g is grouping and f is functional and g.GROUPINGS is grouping.GROUPINGS
