"""The grouping layers on HIP tensors (components/model/layers/grouping.py over csrc/codebook.hip) against the reference's values of
tests/golden/grouping.npz.  Tolerance of the configurations the kernels cover: the float64 evaluation of codebook_bound.grouping_ref lies within its
bound of ANY fp32 evaluation -- the reference's (test_grouping_host.py checks that on the CPU) and the device's -- so the two differ by at most
twice that bound per element.  The fixture's assignment gaps guarantee equal assignments; the ids are compared with the float64 arg-min."""
import os

import numpy as np
import pytest
import torch

import codebook_bound as B
import grouping_fixture as G

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grouping.npz"))
FALLBACKS = {       # configurations outside the kernels: the torch-op formulation on the device
    "soft": G.CASES["soft"][1:6],
    "softmax over features": ("normressoftmaxatt", "top-2", "softmax-2.0", "l2norm", "softmaxassatt"),
    "cmeans": ("iden", "all", "cmeans-2.0", "l2norm", "maxass"),
    "rankserie": ("att", "top-3", "rankserie-2.0", "l2norm", "avgass"),
}


def _flat(imgs):
    return (torch.cat([f for fs, _ in imgs for f in fs]).numpy(), torch.cat([a for _, at in imgs for a in at]).numpy())


def _config(name):
    _, features, nearest, assignment, descriptor, weights, _ = G.CASES[name]
    kind, *base = assignment.split("-")
    dname, *dparam = descriptor.split("-")
    return dict(feature=features, ma=int(nearest.split("-")[1]) if "-" in nearest else 1, assignment=kind, base=float(base[0]) if base else 0.0,
                descriptor=dname, param=float(dparam[0]) if dparam else 0.0, weights=weights)


def _reference_inputs(name):
    """(x, att, centroids, sizes) the float64 evaluation of case ``name`` runs on.  batch: the features' own values do not depend on the centroids
    (iden) and the gaps fix the assignments, so the reference's clusters stand in for the device's; topc: the reduced codebook is a selection of
    rows by weights that are maxima of stored attentions, exact on both sides, replayed here in float64."""
    x, att = _flat(G.images())
    c = G.codebook().numpy()
    if name == "batch":
        return x, att, GOLDEN["kmeans_out"], G.SIZES
    if name == "topc":
        near = B.d2_ref(x, c)[0].argmin(1)
        n_pair = G.SIZES[0] + G.SIZES[1]
        w = np.zeros(G.K)
        np.maximum.at(w, near[:n_pair], att[:n_pair, 0].astype(np.float64))
        order = np.argsort(-w, kind="stable")
        keep = np.isin(near, order[:G.CASES[name][6]["top_centroids"]])
        assert int(keep.sum()) == int(GOLDEN["topc_kept"])
        img = np.repeat(np.arange(len(G.SIZES)), G.SIZES)
        return x[keep], att[keep], c[order[:4]], tuple(int((img[keep] == i).sum()) for i in range(len(G.SIZES)))
    return x, att, c, G.SIZES


@pytest.mark.parametrize("name", [n for n in G.CASES if n != "soft"])
def test_device_path_matches_the_reference_values(cuda_device, name):
    from gandtr_amd import codebook
    from gandtr_amd.components.model.layers import grouping
    layer = G.build(grouping.GROUPINGS, name, cuda_device).to(cuda_device)
    imgs = G.images(cuda_device)
    with torch.no_grad():
        assert layer._device_plan(imgs, getattr(layer, "codebook", imgs[0][0][0])) is not None, "this configuration must take the kernels"
    grouped, weights = G.run(layer, name, imgs)
    x, att, c, sizes = _reference_inputs(name)
    r = B.grouping_ref(x, att, c, sizes, **_config(name))
    qg = B.within(grouped.cpu().numpy() - GOLDEN[name + "_grouped"], np.zeros_like(r["grouped"]), 2 * r["grouped_b"])
    qw = B.within(weights.cpu().numpy() - GOLDEN[name + "_weights"], np.zeros_like(r["weights"]), 2 * r["weights_b"])
    qd = B.within(grouped.cpu().numpy(), r["grouped"], r["grouped_b"])
    print("%s: |device - reference| / (2 bound): grouped %.3f, weights %.3f; |device - float64| / bound %.3f" % (name, qg, qw, qd))
    assert qg <= 1.0 and qw <= 1.0 and qd <= 1.0, (name, qg, qw, qd)
    assert not grouped[1].any() and not weights[1].any()
    if name != "batch":
        _, ids = codebook.nearest(torch.from_numpy(x).to(cuda_device), torch.from_numpy(c).to(cuda_device), r["ids"].shape[1])
        assert np.array_equal(ids.cpu().numpy(), r["ids"]), "the device's ids are the float64 arg-min"


@pytest.mark.parametrize("name", list(FALLBACKS))
def test_fallback_configurations_equal_the_cpu_path(cuda_device, name):
    from gandtr_amd.components.model.layers import grouping
    args = FALLBACKS[name]
    cpu = grouping.LoadedCodebook(G.codebook(), *args, 1.0, 0, outputdim=G.D)
    dev = grouping.LoadedCodebook(G.codebook().to(cuda_device), *args, 1.0, 0, outputdim=G.D).to(cuda_device)
    assert dev._device_plan(G.images(cuda_device), dev.codebook) is None
    with torch.no_grad():
        g0, w0 = cpu._forward(G.images())
        g1, w1 = dev._forward(G.images(cuda_device))
    assert g1.is_cuda and w1.is_cuda
    for got, ref in ((g1, g0), (w1, w0)):
        assert float((got.cpu() - ref).abs().max()) <= 1e-5 * float(ref.abs().max()), name
    if name == "soft":
        assert float(np.abs(g1.cpu().numpy() - GOLDEN["soft_grouped"]).max()) <= 1e-5 * float(np.abs(GOLDEN["soft_grouped"]).max())


def test_a_gradient_request_takes_the_torch_formulation(cuda_device):
    from gandtr_amd.components.model.layers import grouping
    layer = G.build(grouping.GROUPINGS, "normresatt", cuda_device).to(cuda_device)
    imgs = G.images(cuda_device)
    assert layer._device_plan(imgs, layer.codebook) is None                # the codebook is a Parameter and gradients are enabled
    with torch.no_grad():
        assert layer._device_plan(imgs, layer.codebook) is not None
    grouped, _ = layer._forward(imgs)
    grouped.sum().backward()
    assert layer.codebook.grad is not None and bool(torch.isfinite(layer.codebook.grad).all())


def test_iterate_kmeans_on_the_device_against_the_cpu_path(cuda_device):
    from gandtr_amd.components.model.layers import functional
    pts, cen = B.blobs()
    cpu = functional.iterate_kmeans(torch.from_numpy(pts), torch.from_numpy(cen.copy()), 2)
    start = torch.from_numpy(cen.copy()).to(cuda_device)
    dev = functional.iterate_kmeans(torch.from_numpy(pts).to(cuda_device), start, 2)
    assert dev.data_ptr() == start.data_ptr()                                # updated in place, like the reference
    want = B.d2_ref(pts, cen)[0].argmin(1)
    r = B.aggregate_ref(pts, None, cen, want.reshape(-1, 1).astype(np.int32), None, (300,), "iden")
    ref, b = B.mean_ref(r["S"][0], r["E"][0], r["count"][0])
    assert (B.d2_ref(pts, ref[:6].astype(np.float32))[0].argmin(1) == want).all()          # the assignment is stable: both iterations form the same means
    assert B.within(dev.cpu().numpy()[:6] - cpu.numpy()[:6], np.zeros((6, 8)), 2 * b[:6]) <= 1.0
    assert torch.equal(dev.cpu()[6], cpu[6]) and torch.equal(cpu[6], torch.from_numpy(cen[6]))
