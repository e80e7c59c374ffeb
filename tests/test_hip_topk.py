"""Streaming top-k, query expansion and database augmentation on the GPU (gandtr_amd/csrc/retrieval_topk.hip) against the float64 oracle
tests/topk_ref.py.  Row conventions of the C ABI inside the helpers (vecs [ndb][d]); the public functions take D x N like the rest of the module."""
import functools

import numpy as np
import pytest
import torch

import topk_ref as R
from gandtr_amd import retrieval
from gandtr_amd.tools import synth

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _unit_rows(seed, d, n):
    v = synth._normal(seed, "v", (d, n))
    return (v / v.norm(dim=0, keepdim=True)).t().contiguous()


@functools.lru_cache(maxsize=None)
def _tie_case():
    """integers in [-3, 3], d = 40: every score is an integer below 2^11, exact in fp32 and in float64; 300 of the 1500 rows repeat earlier ones"""
    rng = np.random.RandomState(7)
    vecs = rng.randint(-3, 4, (1500, 40)).astype(np.float32)
    vecs[rng.permutation(1200)[:300] + 300] = vecs[rng.randint(0, 300, 300)]
    qvecs = rng.randint(-3, 4, (5, 40)).astype(np.float32)
    return vecs, qvecs


@functools.lru_cache(maxsize=None)
def _tie_ref(k, self_on_db):
    vecs, qvecs = _tie_case()
    return R.ref_topk(vecs, vecs, k, 0) if self_on_db else R.ref_topk(vecs, qvecs, k)


def _dev(a, device):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device)


def _run(vecs, qvecs, k, device, index_base=0, self_base=-1, slices=0):
    s, i = retrieval._topk_rows(_dev(vecs, device), _dev(qvecs, device), k, index_base, self_base, slices)
    return s.cpu().numpy(), i.cpu().numpy()


def _check_valid(scores, ids, s64, k, self_base=-1):
    """the validity rule: what a correct selection on scores known to 2e-6 must satisfy.  s64 [nq][ndb] float64."""
    nq, ndb = s64.shape
    assert scores.shape == (nq, k) and ids.shape == (nq, k) and ids.dtype == np.int32 and scores.dtype == np.float32
    worst = 0.0
    for q in range(nq):
        ref = s64[q].copy()
        if self_base >= 0:
            ref[self_base + q] = -np.inf
        n = min(k, ndb - (1 if self_base >= 0 else 0))
        got_i, got_s = ids[q, :n], scores[q, :n].astype(np.float64)
        assert np.all(ids[q, n:] == -1) and np.all(np.isneginf(scores[q, n:]))                 # fewer than k rows: the tail
        assert np.all(got_i >= 0) and np.all(got_i < ndb) and len(set(got_i.tolist())) == n    # no duplicate ids
        if self_base >= 0:
            assert self_base + q not in got_i
        err = np.abs(got_s - ref[got_i]).max()
        worst = max(worst, err)
        assert err < 2e-6, (q, err)                                                            # the gate of test_hip_retrieval.py
        assert np.all(got_s[:-1] >= got_s[1:])                                                 # never increase
        kth = np.sort(ref)[::-1][n - 1]
        assert np.all(ref[got_i] >= kth - 4e-6), (q, (kth - ref[got_i]).max())                 # two scores, each within 2e-6
    return worst


# ---- 1. exact case with ties

@pytest.mark.parametrize("k", [1, 10, 256])
def test_exact_scores_break_ties_by_id(cuda_device, k):
    vecs, qvecs = _tie_case()
    ref_s, ref_i = _tie_ref(k, False)
    s, i = _run(vecs, qvecs, k, cuda_device)
    assert np.array_equal(i, ref_i) and np.array_equal(s.astype(np.float64), ref_s)
    s, i = _run(vecs, qvecs, k, cuda_device, index_base=1000)
    assert np.array_equal(i, ref_i + 1000) and np.array_equal(s.astype(np.float64), ref_s)
    ref_s, ref_i = _tie_ref(k, True)
    s, i = _run(vecs, vecs, k, cuda_device, self_base=0)                                       # database against itself, no vector its own match
    assert np.array_equal(i, ref_i) and np.array_equal(s.astype(np.float64), ref_s)


# ---- 2. the result does not depend on the slicing

def test_same_bits_for_any_number_of_slices(cuda_device):
    vecs, qvecs = _tie_case()
    cases = [(_dev(vecs, cuda_device), _dev(qvecs, cuda_device), 10), (_dev(vecs, cuda_device), _dev(qvecs, cuda_device), 256),
             (_unit_rows(11, 130, 3001).to(cuda_device), _unit_rows(12, 130, 3).to(cuda_device), 17)]
    for v, q, k in cases:
        base_s, base_i = retrieval._topk_rows(v, q, k, slices=1)
        for slices in (1, 2, 7, 0):
            for _ in range(2):                                                                 # and again on a second run
                s, i = retrieval._topk_rows(v, q, k, slices=slices)
                assert torch.equal(s, base_s) and torch.equal(i, base_i), (k, slices)
    ref_s, ref_i = _tie_ref(256, False)
    s, i = retrieval._topk_rows(cases[1][0], cases[1][1], 256, slices=7)
    assert np.array_equal(i.cpu().numpy(), ref_i) and np.array_equal(s.cpu().numpy().astype(np.float64), ref_s)


# ---- 3. shapes at the edges, 4. validity within rounding (every NB of the scan kernel: k <= 48, <= 112, <= 176, above)

@pytest.mark.parametrize("d,ndb,nq,k", [(1, 300, 9, 5), (7, 1000, 9, 5), (64, 1000, 9, 5), (130, 1000, 9, 5), (24, 5, 3, 8), (130, 3001, 1, 17),
                                        (130, 3001, 70, 17), (2048, 20000, 55, 100),
                                        (96, 4000, 128, 20), (512, 5000, 130, 100), (130, 3001, 64, 150), (64, 3000, 40, 256)])
def test_topk_is_valid_within_rounding(cuda_device, d, ndb, nq, k):
    vecs, qvecs = _unit_rows(1, d, ndb), _unit_rows(2, d, nq)
    s64 = R.ref_scores(vecs.numpy(), qvecs.numpy())
    s, i = _run(vecs, qvecs, k, cuda_device)
    s3, i3 = _run(vecs, qvecs, k, cuda_device, slices=3)             # a forced slicing takes the widest query tile k allows: the same bits
    assert np.array_equal(s, s3) and np.array_equal(i, i3)
    worst = _check_valid(s, i, s64, k)
    print("topk d=%d ndb=%d nq=%d k=%d: max |score - float64| = %.3e" % (d, ndb, nq, k, worst))
    # where the k-th and (k+1)-th float64 scores are further apart than the rounding, the set is the oracle's
    _, ref_i = R.ref_topk(vecs.numpy(), qvecs.numpy(), min(k + 1, ndb))
    for q in range(nq):
        if ndb > k and s64[q, ref_i[q, k - 1]] - s64[q, ref_i[q, k]] > 4e-6:
            assert set(i[q].tolist()) == set(ref_i[q, :k].tolist())


def test_knn_rows_exclude_themselves(cuda_device):
    vecs = _unit_rows(3, 48, 900)
    s64 = R.ref_scores(vecs.numpy(), vecs.numpy()[300:420])
    s, i = _run(vecs, vecs[300:420], 9, cuda_device, self_base=300)
    _check_valid(s, i, s64, 9, self_base=300)


# ---- 5. expand alone

@pytest.mark.parametrize("d", [7, 512])
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("alpha", [0.0, 1.0, 3.0])
def test_expand_matches_float64_under_the_rounding_gate(cuda_device, alpha, k, d):
    """per element (k + 8) * 2^-23 * (|base_i| + sum_j |w_j v_ji|) / ||x||: k + 1 fp32 additions, powf and the norm"""
    vecs, qvecs = _unit_rows(4, d, 400), _unit_rows(5, d, 6)
    v, q = vecs.to(cuda_device), qvecs.to(cuda_device)
    scores, ids = retrieval._topk_rows(v, q, k)                       # the device's own selection: no selection noise in the comparison
    shares = []
    for variant in ("with_base", "no_base", "holes"):
        sc, idx, base = scores.clone(), ids.clone(), q
        if variant == "no_base":
            base = None
        if variant == "holes":                                          # missing entries and negative scores (weight 0 for alpha > 0)
            idx[::2, 0] = -1
            sc[1::2, k // 2] = -0.25
            sc[0, :] = -sc[0, :]
        out = retrieval._expand_rows(v, base, idx, sc, alpha)
        again = retrieval._expand_rows(v, base, idx, sc, alpha)
        assert torch.equal(out, again)                                  # fixed order: the same bits
        ref, mag, norm = R.ref_expand(vecs.numpy(), None if base is None else qvecs.numpy(), idx.cpu().numpy(), sc.cpu().numpy(), alpha)
        gate = (k + 8) * 2.0 ** -23 * mag / norm
        err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
        live = gate > 0
        shares.append(float((err[live] / gate[live]).max()))
        assert np.all(err <= gate), (variant, shares[-1])
    print("expand alpha=%g k=%d d=%d: largest share of the gate %.3f" % (alpha, k, d, max(shares)))


# ---- 6. the public functions

def test_public_functions_equal_the_composition(cuda_device):
    d, ndb, k = 24, 700, 5
    vecs, qvecs = _unit_rows(6, d, ndb).to(cuda_device), _unit_rows(7, d, 33).to(cuda_device)
    V, Q = vecs.t(), qvecs.t()                                          # D x N views, as the module's callers hold them
    s, i = retrieval.topk(V, Q, k, index_base=10)
    rs, ri = retrieval._topk_rows(vecs, qvecs, k, 10)
    assert s.shape == (k, 33) and i.dtype == torch.int32 and torch.equal(s, rs.t()) and torch.equal(i, ri.t())
    rs, ri = retrieval._topk_rows(vecs, qvecs, k)
    for alpha in (3.0, 0.0):
        out = retrieval.expand_queries(V, Q, k, alpha=alpha)
        assert out.shape == (d, 33) and torch.equal(out, retrieval._expand_rows(vecs, qvecs, ri, rs, alpha).t())
    ds, di = retrieval._topk_rows(vecs, vecs, k)
    want = retrieval._expand_rows(vecs, None, di, ds, 3.0).t()
    assert torch.equal(di[:, 0].cpu(), torch.arange(ndb, dtype=torch.int32))      # every vector finds itself first
    for block in (100, 8192):
        out = retrieval.augment_database(V, k, alpha=3.0, block=block)
        assert out.shape == (d, ndb) and torch.equal(out, want), block            # the block size is not observable
    # l2n divides by ||x|| + 1e-6 and ||x|| >= 1 here (the vector itself enters with weight 1, its matches with positive scores)
    for m in (want, retrieval.expand_queries(V, Q, k)):
        assert float((m.double().norm(dim=0) - 1).abs().max()) <= 1e-6
    ks, ki = retrieval.knn_graph(V, k, block=256)
    es, ei = retrieval.topk(V, V, k, exclude_self=True)
    assert torch.equal(ks, es) and torch.equal(ki, ei)
    assert not bool((ki == torch.arange(ndb, device=cuda_device, dtype=torch.int32)[None, :]).any())
    assert torch.equal(ki[:k - 1], di.t()[1:]) and torch.equal(ks[:k - 1], ds.t()[1:])     # the search with itself, minus itself
    with pytest.raises(ValueError):
        retrieval.topk(V, Q, k, exclude_self=True)
    with pytest.raises(ValueError):
        retrieval.topk(V, Q, 257)


def test_query_expansion_pulls_a_query_towards_its_group(cuda_device):
    d, nq = 64, 12
    q = _unit_rows(8, d, nq)
    noise = synth._normal(9, "n", (4 * nq, d))
    group = q.repeat_interleave(4, dim=0) + 0.5 * noise / noise.norm(dim=1, keepdim=True)      # 4 near-duplicates per query
    group = group / group.norm(dim=1, keepdim=True)
    vecs = torch.cat([_unit_rows(10, d, 600), group])
    out = retrieval.expand_queries(vecs.t().to(cuda_device), q.t().to(cuda_device), 4, alpha=3.0).t().cpu()
    before = (q.double()[:, None, :] * group.double().view(nq, 4, d)).sum(-1).mean(1)
    after = (out.double()[:, None, :] * group.double().view(nq, 4, d)).sum(-1).mean(1)
    assert bool((after > before).all()), (before, after)


# ---- 7. a size the score matrix cannot take

def test_topk_beyond_two_to_the_31_scores(cuda_device):
    ndb, nq, d, k = 70000, 32768, 16, 4
    assert ndb * nq > 2 ** 31
    vecs, qvecs = _unit_rows(13, d, ndb), _unit_rows(14, d, nq)
    s, i = retrieval.topk(vecs.t().to(cuda_device), qvecs.t().to(cuda_device), k)
    assert s.shape == (k, nq) and i.shape == (k, nq)
    sample = np.linspace(0, nq - 1, 64).astype(np.int64)
    s64 = R.ref_scores(vecs.numpy(), qvecs.numpy()[sample])
    _check_valid(s.t()[sample].cpu().numpy(), i.t()[sample].cpu().numpy(), s64, k)
