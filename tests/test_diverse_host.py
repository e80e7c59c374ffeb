"""Diverse-anchor mining on the host (no GPU): the torch restatement of ``DiverseAnchorsDataset._select_positive_pairs_db`` against what
the reference's own method returned (tests/golden/diverse_anchors.npz, written by tests/golden/make_diverse_golden.py), the rank
arithmetic against a literal transcription, argument errors, and ``create_epoch_tuples`` against a by-hand composition of its parts."""
import os

import numpy as np
import pytest
import torch

from gandtr_amd import mining, retrieval

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diverse_anchors.npz")


def load_cases():
    g = np.load(GOLDEN)
    cases = []
    for k in range(int(g["cases"])):
        c = {key[len("c%d_" % k):]: g[key] for key in g.files if key.startswith("c%d_" % k)}
        c["mark_easy"] = None if np.isnan(c["mark_easy"]) else float(c["mark_easy"])
        for key in ("seed", "qpool", "qsize", "nnum", "randint_after"):
            c[key] = int(c[key])
        for key in ("exclude", "include"):
            c[key] = float(c[key])
        c["shuffle"], c["dup"] = bool(c["shuffle"]), bool(c["dup"])
        cases.append(c)
    return cases


def run_case(c, device=None):
    """the case through mining.select_positive_pairs_diverse, seeded as the generator seeded the reference"""
    vecs = torch.from_numpy(c["vecs"])
    if device is not None:
        vecs = vecs.to(device)
    db = {"qidxs": c["db_qidxs"].tolist(), "pidxs": c["db_pidxs"].tolist()}
    labels_seen = []

    def extract(idxs, label):
        labels_seen.append(label)
        return vecs[:, idxs]
    torch.manual_seed(c["seed"])
    out = mining.select_positive_pairs_diverse(db, c["qsize"], c["qpool"], c["exclude"], c["include"], c["shuffle"], extract,
                                               mark_easy=c["mark_easy"], first_neg="neg", nnum=c["nnum"])
    after = int(torch.randint(2 ** 31, (1,)).item())
    return out, after, labels_seen


def check_case(c, out, after):
    qidxs, pidxs, labels, meta = out
    assert qidxs == c["qidxs"].tolist()
    assert pidxs == c["pidxs"].tolist()
    assert labels == c["labels"].tolist()
    assert set(meta) == {"average_new_query_max_score"}
    got = np.array(meta["average_new_query_max_score"])
    assert got.shape == c["scores"].shape
    err = float(np.abs(got - c["scores"]).max())
    print("max |score - reference| = %.3e" % err)
    assert err <= 1e-6
    assert after == c["randint_after"]                     # the generator is left where the reference leaves it


def test_fixture_covers_what_it_must():
    cases = load_cases()
    assert any(c["mark_easy"] is not None for c in cases)
    assert any(c["shuffle"] and c["qpool"] < len(c["db_qidxs"]) for c in cases)
    assert any(c["qsize"] == c["qpool"] for c in cases)
    for c in cases:
        assert float(c["min_gap"]) >= 2e-5
        if c["dup"]:                                         # an exact duplicate of the first anchor's vector inside the pool
            torch.manual_seed(c["seed"])
            pool = mining._randperm(len(c["db_qidxs"]), c["qpool"], c["shuffle"])
            v = c["vecs"][:, c["db_qidxs"][pool]]
            assert np.array_equal(v[:, 0], v[:, c["qpool"] // 2])
    assert any(c["dup"] for c in cases)
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("k", range(4))
def test_host_path_matches_the_reference(k):
    c = load_cases()[k]
    out, after, labels_seen = run_case(c)
    check_case(c, out, after)
    assert labels_seen == (["anc-pool"] if c["mark_easy"] is None else ["anc-pool", "pos-pool"])


def _targets_literal(qpool_size, qsize, similar_exclude, similar_include):
    """cirtorch_datasets.py:88-95 with shuffle off, step by step as written there"""
    idxs, out = [0], []
    for _ in range(qsize - 1):
        valid_size = qpool_size - len(idxs)
        similar_split = max(int(valid_size * (1 - similar_exclude)), 1)
        dissimilar_split = min(int(valid_size * (1 - similar_include)), similar_split - 1)
        dissimilar_part = list(range(qpool_size))[dissimilar_split:similar_split]
        out.append(dissimilar_part[len(dissimilar_part) - 1])
        idxs.append(out[-1])
    return out


@pytest.mark.parametrize("qpool,qsize,ex,inc", [(50, 20, 0.5, 0.5), (50, 20, 0.0, 0.3), (37, 37, 0.2, 0.8), (37, 37, 0.0, 1.0), (10, 10, 1.0, 1.0),
                                                (2, 2, 0.3, 0.6), (1000, 200, 0.1, 0.9)])
def test_targets_against_a_literal_transcription(qpool, qsize, ex, inc):
    got = retrieval.diverse_anchor_targets(qpool, qsize, ex, inc, False)
    assert got.dtype == torch.int64 and got.shape == (qsize - 1,)
    assert got.tolist() == _targets_literal(qpool, qsize, ex, inc)
    # with shuffle: one randint per step over the same slice, in step order
    torch.manual_seed(5)
    shuffled = retrieval.diverse_anchor_targets(qpool, qsize, ex, inc, True)
    torch.manual_seed(5)
    for t in range(qsize - 1):
        valid = qpool - (t + 1)
        sim = max(int(valid * (1 - ex)), 1)
        dis = min(int(valid * (1 - inc)), sim - 1)
        assert int(shuffled[t]) == dis + torch.randint(sim - dis, (1,)).item()
        assert 0 <= int(shuffled[t]) < qpool


def test_ties_rank_by_lower_index():
    """columns 1 and 3 are the same vector: whenever their shared similarity is the target, the lower column is taken first"""
    v = torch.tensor([[1.0, 0.6, 0.0, 0.6, -1.0], [0.0, 0.8, 1.0, 0.8, 0.0]])
    idxs, scores = retrieval._diverse_anchors_host(v, torch.tensor([2]))
    assert idxs == [0, 1] and scores == [pytest.approx(0.6)]
    idxs, _ = retrieval._diverse_anchors_host(v, torch.tensor([3]))
    assert idxs == [0, 3]


def test_argument_errors():
    v = torch.nn.functional.normalize(torch.randn(8, 12, generator=torch.Generator().manual_seed(0)), dim=0)
    with pytest.raises(ValueError):
        retrieval.select_diverse_anchors(v, 1, 0.2, 0.8, False)
    with pytest.raises(ValueError):
        retrieval.select_diverse_anchors(v, 13, 0.2, 0.8, False)
    with pytest.raises(AssertionError):
        retrieval.select_diverse_anchors(v, 4, 0.8, 0.2, False)
    with pytest.raises(ValueError):                                    # the device chain takes device descriptors only: no silent host run
        retrieval.diverse_anchors(v, [3, 2, 1])
    db = {"qidxs": list(range(12)), "pidxs": list(range(12)), "cluster": [0] * 12}
    with pytest.raises(AssertionError):
        mining.select_positive_pairs_diverse(db, 6, 4, 0.2, 0.8, False, lambda idxs, label: v[:, idxs])
    with pytest.raises(ValueError):
        mining.select_positive_pairs_diverse(db, 6, 20, 0.2, 0.8, False, lambda idxs, label: v[:, idxs])
    idxs, scores = retrieval.select_diverse_anchors(v, 12, 0.2, 0.8, False)
    assert len(idxs) == 12 and len(scores) == 11 and idxs[0] == 0


def _host_hard_negatives(qidxs, qvecs, idxs2images, poolvecs, clusters, nnum):
    """traindataset.py:246-279 on the host (oracle/retrieval_oracle.py)"""
    from oracle import retrieval_oracle as R
    nidxs, dist = R.search_hard_negatives(list(qidxs), qvecs.numpy(), list(idxs2images), poolvecs.numpy(), list(clusters), nnum)
    return [list(map(int, n)) for n in nidxs], {"average_negative_distance": [float(x) for x in np.asarray(dist).reshape(-1)]}


@pytest.mark.parametrize("shuffle,mark_easy,nnum", [(True, 0.3, 3), (False, None, 2), (True, None, 0)])
def test_create_epoch_tuples_is_the_composition_of_its_parts(monkeypatch, shuffle, mark_easy, nnum):
    monkeypatch.setattr(retrieval, "search_hard_negatives", _host_hard_negatives)
    nimg, npairs, d = 240, 150, 16
    rng = np.random.RandomState(3)
    vecs = torch.nn.functional.normalize(torch.from_numpy(rng.randn(d, nimg).astype(np.float32)), dim=0)
    db = {"qidxs": rng.permutation(nimg)[:npairs].tolist(), "pidxs": rng.permutation(nimg)[:npairs].tolist(),
          "cluster": rng.randint(0, 30, nimg).tolist()}
    calls = []

    def extract(idxs, label):
        calls.append((len(idxs), label if isinstance(label, str) else list(label)))
        return vecs[:, idxs]
    kw = dict(qsize=25, poolsize=90, nnum=nnum, qpool_size=400, similar_exclude=0.1, similar_include=0.9, shuffle=shuffle, mark_easy=mark_easy)
    torch.manual_seed(11)
    qidxs, pidxs, nidxs, labels, meta = mining.create_epoch_tuples(db, [None] * nimg, None, 64, None, extract=extract, **kw)
    state = torch.randint(2 ** 31, (1,)).item()
    # by hand, in the reference's order of draws: pool permutation, choices, negative-pool permutation
    torch.manual_seed(11)
    qpool = min(400, npairs)                                            # the constructor's cap
    pool = torch.randperm(npairs)[:qpool].tolist() if shuffle else list(range(qpool))
    pq, pp = [db["qidxs"][i] for i in pool], [db["pidxs"][i] for i in pool]
    idxs, acc = retrieval.select_diverse_anchors(vecs[:, pq], 25, 0.1, 0.9, shuffle)
    want_q, want_p = [pq[i] for i in idxs], [pp[i] for i in idxs]
    assert (qidxs, pidxs) == (want_q, want_p)
    assert meta["average_new_query_max_score"] == acc
    heads = ["anc", "pos", "neg"] + ["neg"] * (nnum - 1)               # the reference's list: three labels even without negatives
    assert len(labels) == len(heads) and all(len(row) == 25 for row in labels)
    if mark_easy is None:
        assert [row[0] for row in labels] == heads
    else:
        sims = (vecs[:, want_q] * vecs[:, want_p]).sum(0)
        easy = set(sims.argsort()[-int(mark_easy * 25):].tolist())
        assert labels[0] == ["anc-easy" if i in easy else "anc-hard" for i in range(25)]
        assert sum(x == "anc-easy" for x in labels[0]) == int(mark_easy * 25)
        assert [x[3:] for x in labels[0]] == [x[3:] for x in labels[1]] == [x[3:] for x in labels[2]]
    if nnum == 0:
        assert nidxs == [[] for _ in range(25)] and set(meta) == {"average_new_query_max_score"}
    else:
        images = torch.randperm(nimg)[:90].tolist() if shuffle else list(range(90))
        want_n, neg_meta = _host_hard_negatives(want_q, vecs[:, want_q], images, vecs[:, images], db["cluster"], nnum)
        assert nidxs == want_n and meta["average_negative_distance"] == neg_meta["average_negative_distance"]
        assert set(meta) == {"average_new_query_max_score", "average_negative_distance"}
        assert calls[-2:] == [(25, labels[0]), (90, "neg-pool")]
        for q, negs in zip(qidxs, nidxs):                              # the cluster rules of the negatives
            cl = [db["cluster"][n] for n in negs]
            assert len(negs) == nnum and len(set(cl)) == nnum and db["cluster"][q] not in cl
    assert state == torch.randint(2 ** 31, (1,)).item()


def test_c_entry_rejects_bad_arguments_before_any_device_call():
    """the argument checks of gdt_retrieval_diverse_anchors come first, so they run on a host without a GPU (the pointers are never read)"""
    import ctypes
    from gandtr_amd import _hip
    lib = _hip.load()
    need = ctypes.c_size_t()
    _hip.check(lib.gdt_retrieval_diverse_anchors_workspace_bytes(100, 37, 10, ctypes.byref(need)))
    assert need.value >= 100 * 4
    for nq, d, nsel in ((1, 8, 2), (100, 0, 10), (100, 8, 1), (100, 8, 101)):
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_retrieval_diverse_anchors_workspace_bytes(nq, d, nsel, ctypes.byref(need)))
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_retrieval_diverse_anchors_workspace_bytes(100, 8, 10, None))
    p = 1 << 20                                                         # stands for a device address
    ok = dict(vecs=p, nq=100, d=37, target=p, nsel=10, first=0, idx=p, score=p, ws=p, ws_bytes=need.value)
    for change in (dict(vecs=None), dict(target=None), dict(idx=None), dict(score=None), dict(ws=None), dict(nsel=1), dict(nsel=101),
                   dict(first=-1), dict(first=100), dict(ws_bytes=need.value - 1), dict(ws_bytes=0), dict(nq=1, nsel=2, first=0), dict(d=0)):
        a = dict(ok, **change)
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_retrieval_diverse_anchors(a["vecs"], a["nq"], a["d"], a["target"], a["nsel"], a["first"], a["idx"], a["score"],
                                                         a["ws"], a["ws_bytes"], None))
