"""Diverse-anchor mining on the device (gdt_retrieval_diverse_anchors, gandtr_amd/mining.py).

Small cases: the reference's own results (tests/golden/diverse_anchors.npz), exact -- the fixture only holds cases whose picks keep a
distance of 2e-5 from their neighbours, more than fp32 rounding can move them.  At the scenario's sizes the smallest distance between
neighbours is about 4e-8, below fp32 rounding, so exact agreement with any other summation order is not a valid demand there: the device's
own chain is replayed in float64 and EVERY step must be a valid pick within eps = 2 * d * 2^-24 (a dot product of unit vectors carries an
error of at most d * 2^-24 on either side of the comparison)."""
import copy
import pickle

import numpy as np
import pytest
import torch

from gandtr_amd.tools import synth
from test_diverse_host import check_case, load_cases, run_case

pytestmark = pytest.mark.gpu


def clustered_unit_vectors(seed, d, n):
    rng = np.random.RandomState(seed)
    ncl = max(n // 10, 4)
    centres = rng.randn(d, ncl).astype(np.float32)
    v = centres[:, rng.randint(0, ncl, n)] + 0.7 * rng.randn(d, n).astype(np.float32)
    return (v / np.linalg.norm(v, axis=0, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("k", range(4))
def test_kernel_matches_the_reference(cuda_device, k):
    c = load_cases()[k]
    out, after, _ = run_case(c, cuda_device)
    check_case(c, out, after)


def replay_and_check(vecs, targets, idxs, scores):
    """float64 replay of the device's own picks; every step is asserted"""
    d, nq = vecs.shape
    eps = 2 * d * 2.0 ** -24
    v64 = vecs.astype(np.float64)
    rows = np.ascontiguousarray(v64.T)
    ms = np.full(nq, -np.inf)
    assert idxs[0] == 0 and len(idxs) == len(targets) + 1 and len(scores) == len(targets)
    worst_score, slack = 0.0, []
    for t, target in enumerate(targets):
        assert 0 <= idxs[t + 1] < nq
        ms = np.maximum(ms, rows @ v64[:, idxs[t]])
        v = ms[idxs[t + 1]]
        below, upto = int((ms < v - eps).sum()), int((ms <= v + eps).sum())
        assert below <= target <= upto - 1, "step %d: target %d outside [%d, %d]" % (t, target, below, upto - 1)
        err = abs(scores[t] - v)
        assert err <= eps, "step %d: score off by %.3e" % (t, err)
        worst_score = max(worst_score, err)
        slack.append(upto - 1 - below)
    print("d=%d nq=%d steps=%d: max |score - float64| = %.3e (eps %.3e), widest admissible window %d positions"
          % (d, nq, len(targets), worst_score, eps, max(slack)))


@pytest.mark.parametrize("d", [512, 100])
def test_property_scenario_pool(cuda_device, d):
    """the fine-tuning scenario's pool: 2000 anchors of 10000, shuffle off"""
    from gandtr_amd import retrieval
    vecs = clustered_unit_vectors(1, d, 10000)
    targets = retrieval.diverse_anchor_targets(10000, 2000, 0.2, 0.8, False)
    idxs, scores = retrieval.diverse_anchors(torch.from_numpy(vecs).to(cuda_device), targets)
    replay_and_check(vecs, targets.tolist(), idxs.cpu().tolist(), scores.cpu().double().tolist())


@pytest.mark.parametrize("d", [2048, 100])
def test_property_shuffled_odd_pool(cuda_device, d):
    from gandtr_amd import retrieval
    vecs = clustered_unit_vectors(2, d, 4099)
    torch.manual_seed(7)
    targets = retrieval.diverse_anchor_targets(4099, 1000, 0.1, 0.9, True)
    idxs, scores = retrieval.diverse_anchors(torch.from_numpy(vecs).to(cuda_device), targets)
    replay_and_check(vecs, targets.tolist(), idxs.cpu().tolist(), scores.cpu().double().tolist())


def test_scalar_load_path_and_ties(cuda_device):
    """d not a multiple of four (no float4 loads) and exact duplicates: equal similarities rank by lower index, as on the host"""
    from gandtr_amd import retrieval
    vecs = clustered_unit_vectors(3, 37, 500)
    vecs[:, 250:500] = vecs[:, 0:250]                                   # every vector twice: each target sits in a tie of two
    torch.manual_seed(9)
    targets = retrieval.diverse_anchor_targets(500, 120, 0.1, 0.9, True)
    idxs, scores = retrieval.diverse_anchors(torch.from_numpy(vecs).to(cuda_device), targets)
    idxs, scores = idxs.cpu().tolist(), scores.cpu().double().tolist()
    replay_and_check(vecs, targets.tolist(), idxs, scores)
    # columns i and i + 250 go through the same arithmetic and always carry the same bits: where such a pair stands clear of its
    # neighbours (1e-4, far above rounding) it holds two known positions, and the lower column must hold the lower one
    checked = 0
    v64 = vecs.astype(np.float64)
    ms = np.full(500, -np.inf)
    for t, target in enumerate(targets.tolist()):
        ms = np.maximum(ms, v64.T @ v64[:, idxs[t]])
        lo = idxs[t + 1] % 250
        rank_lo = int((ms < ms[lo]).sum())                             # float64 position of the pair's first member
        if abs(np.sort(ms)[max(rank_lo - 1, 0)] - ms[lo]) > 1e-4 and (rank_lo + 2 >= 500 or abs(np.sort(ms)[rank_lo + 2] - ms[lo]) > 1e-4):
            # the pair is isolated: it occupies positions rank_lo (lower column) and rank_lo + 1 (upper column)
            assert target in (rank_lo, rank_lo + 1), "step %d" % t
            assert idxs[t + 1] == (lo if target == rank_lo else lo + 250), "step %d" % t
            checked += 1
    assert checked >= 60, checked


def test_repeatable_streams_and_views(cuda_device):
    from gandtr_amd import retrieval
    vecs = torch.from_numpy(clustered_unit_vectors(4, 96, 1500)).to(cuda_device)
    torch.manual_seed(3)
    targets = retrieval.diverse_anchor_targets(1500, 300, 0.2, 0.8, True)
    a_idx, a_sc = retrieval.diverse_anchors(vecs, targets)
    b_idx, b_sc = retrieval.diverse_anchors(vecs, targets)
    assert torch.equal(a_idx, b_idx) and torch.equal(a_sc.view(torch.int32), b_sc.view(torch.int32))     # bit for bit
    side = torch.cuda.Stream(device=cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(side):
        c_idx, c_sc = retrieval.diverse_anchors(vecs, targets)
    side.synchronize()
    assert torch.equal(a_idx, c_idx) and torch.equal(a_sc.view(torch.int32), c_sc.view(torch.int32))
    wide = torch.zeros((96, 3000), device=cuda_device)
    wide[:, ::2] = vecs
    view = wide[:, ::2]                                                  # D x Q with a column stride of two
    assert not view.is_contiguous() and not view.t().is_contiguous()
    d_idx, d_sc = retrieval.diverse_anchors(view, targets)
    assert torch.equal(a_idx, d_idx) and torch.equal(a_sc.view(torch.int32), d_sc.view(torch.int32))
    # another first anchor: the chain starts there
    e_idx, _ = retrieval.diverse_anchors(vecs, targets, first_idx=17)
    assert int(e_idx[0]) == 17
    # the high-level call agrees with the explicit one (shuffle off: no draws involved)
    idxs, acc = retrieval.select_diverse_anchors(vecs, 300, 0.2, 0.8, shuffle=False)
    f_idx, f_sc = retrieval.diverse_anchors(vecs, retrieval.diverse_anchor_targets(1500, 300, 0.2, 0.8, False))
    assert idxs == f_idx.cpu().tolist() and acc == f_sc.cpu().tolist()


def test_bad_target_raises_before_any_launch(cuda_device):
    from gandtr_amd import retrieval
    vecs = torch.from_numpy(clustered_unit_vectors(5, 16, 64)).to(cuda_device)
    for bad in ([3, 64, 2], [3, -1, 2], [], list(range(64))):
        with pytest.raises(ValueError):
            retrieval.diverse_anchors(vecs, bad)
    with pytest.raises(ValueError):
        retrieval.diverse_anchors(vecs, [1, 2], first_idx=64)
    with pytest.raises(ValueError):
        retrieval.select_diverse_anchors(vecs, 65, 0.2, 0.8)
    with pytest.raises(ValueError):
        retrieval.select_diverse_anchors(vecs, 1, 0.2, 0.8)


# ---- create_epoch_tuples end to end on image files (the set-up of tests/test_hip_map.py's validate test)

SIZES = [(72, 96), (96, 72), (80, 80), (64, 104), (88, 64)]


def _jpeg(path, seed, hw):
    from PIL import Image
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.02, 0.2, (3, 2))
    ph = rng.uniform(0, 6.3, 3)
    img = np.stack([127 + 100 * np.sin(f[c, 0] * yy + f[c, 1] * xx + ph[c]) for c in range(3)], -1)
    img += rng.normal(0, 12, img.shape)
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8), "RGB").save(path, "JPEG", quality=90)


def _network(tmp_path, device):
    import hubconf
    from gandtr_amd.learning import load_network
    base = hubconf.gem_vgg16_cyclegan(pretrained=False, device="cpu")
    base.model.load_state_dict(synth.vgg16_state(0))
    sd = base.state_dict()["net"]
    sd["network_params"]["runtime"]["data"] = {"transforms": "pil2np | totensor | normalize",
                                               "mean_std": [[0.485, 0.456, 0.406], [0.229, 0.224, 0.225]]}
    ck = str(tmp_path / "vgg.pth")
    torch.save(sd, ck)
    net = load_network(copy.deepcopy({"path": ck, "runtime": {"wrappers": "cirfaketuplebatch"}}), device).eval()
    return net, net.network_params.runtime["data"]["mean_std"]


def test_create_epoch_tuples_end_to_end(cuda_device, tmp_path):
    from gandtr_amd import mining, retrieval
    from gandtr_amd.stages.validate import extract_vectors_from_files
    nimg = 60
    images = [str(tmp_path / ("img_%02d.jpg" % i)) for i in range(nimg)]
    for i, path in enumerate(images):
        _jpeg(path, i, SIZES[i % len(SIZES)])
    db = {"qidxs": list(range(0, 40)), "pidxs": [(i + 7) % nimg for i in range(40)], "cluster": [i // 3 for i in range(nimg)]}
    with open(tmp_path / "db.pkl", "wb") as f:                            # the reference unpickles this dict; it is used as it is
        pickle.dump(db, f)
    net, mean_std = _network(tmp_path, cuda_device)
    kw = dict(qsize=10, poolsize=50, nnum=3, qpool_size=30, similar_exclude=0.2, similar_include=0.8)
    for shuffle in (False, True):
        torch.manual_seed(1)
        qidxs, pidxs, nidxs, labels, meta = mining.create_epoch_tuples(db, images, net, 96, mean_std, shuffle=shuffle, mark_easy=0.5, **kw)
        assert len(qidxs) == len(pidxs) == len(nidxs) == 10
        pairs = dict(zip(db["qidxs"], db["pidxs"]))
        assert all(pairs[q] == p for q, p in zip(qidxs, pidxs))
        assert len(labels) == 5 and all(len(row) == 10 for row in labels)
        assert sum(x == "anc-easy" for x in labels[0]) == 5 and sum(x == "anc-hard" for x in labels[0]) == 5
        assert len(meta["average_new_query_max_score"]) == 9 and len(meta["average_negative_distance"]) == 30
        for q, negs in zip(qidxs, nidxs):                                  # the cluster rules of the negatives
            cl = [db["cluster"][n] for n in negs]
            assert len(negs) == 3 and len(set(cl)) == 3 and db["cluster"][q] not in cl
            assert all(0 <= n < (nimg if shuffle else 50) for n in negs)
        if not shuffle:                                                    # the anchors: the selection on separately extracted descriptors
            with torch.no_grad():
                qvecs = extract_vectors_from_files(net, [images[i] for i in db["qidxs"][:30]], 96, mean_std)
            idxs, acc = retrieval.select_diverse_anchors(qvecs, 10, 0.2, 0.8, shuffle=False)
            assert qidxs == [db["qidxs"][i] for i in idxs]
            assert np.allclose(meta["average_new_query_max_score"], acc, rtol=0, atol=1e-5)
