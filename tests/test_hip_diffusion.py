"""Diffusion re-ranking on the GPU (gandtr_amd/csrc/retrieval_diffusion.hip) against the float64 restatement tests/diffusion_ref.py.  Row conventions of
the C ABI inside the helpers (ids [n][k]); the public functions take k x N / D x N like the rest of the module.  Every reference is built from the
device's own kNN lists, so the choice between near-tied neighbours cannot matter."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import diffusion_ref as R
from gandtr_amd import _hip, retrieval

pytestmark = pytest.mark.gpu

GAMMA, ALPHA, TOL, MAX_ITER = 3.0, 0.99, 1e-5, 64
AFFINITY_GATE = 68 * 2.0 ** -24            # powf at 16 ulp, the same again through both degrees at half weight each, two roundings of r, two multiplies
SOLVER_SHAPES = [(300, 16, 5, 0.3, 8, 4, 5), (600, 32, 12, 0.5, 10, 5, 7), (3000, 64, 40, 0.6, 20, 10, 70), (300, 16, 5, 0.3, 8, 4, 1)]


def _np(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _graph(n, d, clusters, noise, k):
    """device kNN lists and affinity of a seeded clustered set, and their float64 counterparts: all as [n][k] numpy rows, computed once"""
    dev = torch.device("cuda:0")
    vecs = torch.from_numpy(R.clustered(n, n, d, clusters, noise)).to(dev)
    sc, ids = retrieval.knn_graph(vecs.t(), k)
    w = retrieval.mutual_knn_affinity(sc, ids, GAMMA)
    sc_r, ids_r, w_r = _np(sc.t()), _np(ids.t()), _np(w.t())
    w64, S64, deg = R.affinity(sc_r, ids_r, GAMMA)
    return {"vecs": vecs, "scores": sc, "ids": ids, "weights": w, "scores_r": sc_r, "ids_r": ids_r, "S": w_r, "w64": w64, "S64": S64, "deg": deg,
            "Sd": R.dense(w_r.astype(np.float64), ids_r)}


@functools.lru_cache(maxsize=None)
def _queries(n, d, clusters, noise, k, kq, nq):
    """device top-k seeds of seeded query vectors: (seed_ids kq x nq, seed_w kq x nq on the device, y [n][nq] float64 from those fp32 weights)"""
    g = _graph(n, d, clusters, noise, k)
    qv = torch.from_numpy(R.clustered(n + 1, nq, d, clusters, noise)).to(g["vecs"].device)
    s, sid = retrieval.topk(g["vecs"].t(), qv.t(), kq)
    sw = s.clamp_min(0).pow(GAMMA)
    return qv, s, sid, sw, R.seeds(_np(sid.t()), _np(sw.t()), n)


def _check_affinity(ids, S, S64, w64, deg):
    """exact: symmetric bit for bit, 0 where not mutual, isolated rows 0; values within the gate.  Returns the largest share of the gate."""
    n, k = ids.shape
    assert S.shape == (n, k) and S.dtype == np.float32
    pairs = 0
    for i in range(n):
        for s in range(k):
            j = int(ids[i, s])
            t = np.nonzero(ids[j] == i)[0] if 0 <= j < n else np.zeros(0, dtype=np.int64)
            if t.size:
                assert S[i, s].tobytes() == S[j, t[0]].tobytes(), (i, s, j, int(t[0]))
                pairs += 1
            else:
                assert S[i, s] == 0 and w64[i, s] == 0, (i, s)
    assert np.all(S[deg == 0] == 0)
    err = np.abs(S.astype(np.float64) - S64)
    assert np.all(err <= AFFINITY_GATE * np.abs(S64)), float((err[S64 > 0] / S64[S64 > 0]).max() / AFFINITY_GATE)
    return pairs, (float((err[S64 > 0] / S64[S64 > 0]).max() / AFFINITY_GATE) if (S64 > 0).any() else 0.0)


# ---- 1. affinity

@pytest.mark.parametrize("n,d,k", [(300, 16, 8), (5, 16, 8), (300, 16, 1), (400, 16, 256)])
def test_affinity_is_symmetric_bit_for_bit_and_within_the_rounding_gate(cuda_device, n, d, k):
    g = _graph(n, d, 5, 0.3, k)
    if k > n - 1:
        assert np.all(g["ids_r"][:, n - 1:] == -1)                                              # the -1 tail
    pairs, share = _check_affinity(g["ids_r"], g["S"], g["S64"], g["w64"], g["deg"])
    print("affinity n=%d k=%d: %d mutual slots, largest share of the 68 x 2^-24 gate %.3f" % (n, k, pairs, share))
    assert pairs > 0
    again = retrieval.mutual_knn_affinity(g["scores"], g["ids"], GAMMA)
    assert torch.equal(again, g["weights"])


def test_affinity_on_a_hand_written_graph_with_holes(cuda_device):
    """a non-mutual edge, an isolated node, a -1 tail and an id outside the database (tests/test_diffusion_host.py's graph)"""
    ids = np.array([[1, -1, -1], [0, 2, -1], [1, -1, -1], [0, -1, -1], [-1, -1, -1], [4, 9, -1]], dtype=np.int32)
    sc = np.array([[0.9, -np.inf, -np.inf], [0.9, 0.5, -np.inf], [0.6, -np.inf, -np.inf], [0.8, -np.inf, -np.inf], [-np.inf] * 3,
                   [0.7, 0.7, -np.inf]], dtype=np.float32)
    w = retrieval.mutual_knn_affinity(torch.from_numpy(sc).to(cuda_device).t(), torch.from_numpy(ids).to(cuda_device).t(), 2.0)
    w64, S64, deg = R.affinity(sc, ids, 2.0)
    S = _np(w.t())
    _check_affinity(ids, S, S64, w64, deg)
    assert np.all(S[3:] == 0) and np.all(np.isfinite(S)) and (S[:3] > 0).sum() == 4


# ---- 2. solver against the dense float64 solve

@pytest.mark.parametrize("n,d,clusters,noise,k,kq,nq", SOLVER_SHAPES)
def test_solver_meets_the_residual_and_error_bounds(cuda_device, n, d, clusters, noise, k, kq, nq):
    g = _graph(n, d, clusters, noise, k)
    _, _, sid, sw, y = _queries(n, d, clusters, noise, k, kq, nq)
    Sd = g["Sd"]
    assert np.array_equal(Sd, Sd.T)
    # the condition, from the reference alone: float64 CG on this system reaches tol within max_iter / 2
    _, its64, res64 = R.cg(Sd, y, ALPHA, TOL, MAX_ITER)
    assert its64.max() <= MAX_ITER // 2 and np.all(res64 <= TOL), its64.max()
    out = retrieval.diffuse(g["weights"], g["ids"], sid, sw, ALPHA, TOL, MAX_ITER)
    f, its, res = _np(out.scores).astype(np.float64), _np(out.iterations), _np(out.residual)
    assert out.scores.shape == (n, nq) and out.scores.dtype == torch.float32 and out.iterations.dtype == torch.int32 and its.shape == (nq,)
    assert np.all(np.isfinite(f)) and np.all(its >= 1) and np.all(its <= MAX_ITER)
    assert np.all(res <= TOL), res.max()
    true = R.true_residual(Sd, y, f, ALPHA)
    ynorm = np.linalg.norm(y, axis=0)
    err = np.linalg.norm(f - R.solve(Sd, y, ALPHA), axis=0)
    print("solver n=%d nq=%d: iterations %d .. %d (float64 CG %d .. %d), true residual / tol at most %.3f, error / bound at most %.3f"
          % (n, nq, its.min(), its.max(), its64.min(), its64.max(), (true / TOL).max(), (err / (true * ynorm / (1 - ALPHA))).max()))
    assert np.all(true <= 3 * TOL), (true / TOL).max()
    assert np.all(err <= true * ynorm / (1 - ALPHA))


# ---- 3. edges

def test_edges_empty_columns_isolated_nodes_duplicate_seeds_and_one_iteration(cuda_device):
    n, k = 300, 8
    g = _graph(n, 16, 5, 0.3, k)
    ids = g["ids"].clone()
    w = g["weights"].clone()
    iso = [7, 123]                                                       # cut two nodes out of the graph: their rows and every edge into them
    for node in iso:
        w[:, node] = 0
        w[ids == node] = 0
    dev = cuda_device
    sid = torch.tensor([[5, 5, 40], [-1, n, -7], [7, 60, 61], [200, 201, 202], [5, 40, -1]], dtype=torch.int32, device=dev).t().contiguous()
    sw = torch.tensor([[1.0, 0.5, 0.25], [1.0, 1.0, 1.0], [2.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.5, 0.25, 9.0]], dtype=torch.float32, device=dev).t().contiguous()
    out = retrieval.diffuse(w, ids, sid, sw, ALPHA, TOL, MAX_ITER)
    f, its, res = _np(out.scores), _np(out.iterations), _np(out.residual)
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(res))
    assert not f[:, 1].any() and its[1] == 0 and res[1] == 0             # no valid seed: exact zeros, 0 iterations, no 0/0
    assert np.all(f[123] == 0) and np.all(f[7, [0, 1, 3, 4]] == 0)       # isolated nodes stay exactly 0 ...
    Sd = R.dense(_np(w.t()).astype(np.float64), g["ids_r"])
    y = R.seeds(_np(sid.t()), _np(sw.t()), n)
    want = R.solve(Sd, y, ALPHA)
    assert abs(want[7, 2] - 2.0) < 1e-12 and f[7, 2] > 1.0                          # ... unless seeded: then the seed stays where it is (bound: next line)
    assert np.all(np.linalg.norm(f - want, axis=0) <= 3 * TOL * np.linalg.norm(y, axis=0) / (1 - ALPHA))
    assert np.array_equal(f[:, 0], f[:, 4]) and its[0] == its[4]         # duplicate seed ids add: (5: 1 + 0.5, 40: 0.25) is (5: 1.5, 40: 0.25)
    one = retrieval.diffuse(w, ids, sid, sw, ALPHA, TOL, 1)
    its1, res1 = _np(one.iterations), _np(one.residual)
    assert np.array_equal(its1, [1, 0, 1, 1, 1]) and np.all(res1[[0, 2, 3, 4]] > TOL) and res1[1] == 0
    with pytest.raises(ValueError):
        retrieval.diffuse(w, ids, sid, sw, 1.0, TOL, MAX_ITER)
    with pytest.raises(ValueError):
        retrieval.diffuse(w, ids, sid, sw, ALPHA, TOL, MAX_ITER, block=65)


# ---- 4. bits

def test_same_bits_for_any_block_any_company_and_any_run(cuda_device):
    shape = SOLVER_SHAPES[2]
    n, d, clusters, noise, k, kq, nq = shape
    g = _graph(n, d, clusters, noise, k)
    _, _, sid, sw, _ = _queries(*shape)
    base = retrieval.diffuse(g["weights"], g["ids"], sid, sw, ALPHA, TOL, MAX_ITER, block=64)
    for block in (1, 7, 64):
        out = retrieval.diffuse(g["weights"], g["ids"], sid, sw, ALPHA, TOL, MAX_ITER, block=block)
        for a, b in zip(out, base):
            assert torch.equal(a, b), block
    for col in (0, 33, 69):                                              # a column alone against the same column among 69 others
        alone = retrieval.diffuse(g["weights"], g["ids"], sid[:, col:col + 1], sw[:, col:col + 1], ALPHA, TOL, MAX_ITER)
        assert torch.equal(alone.scores[:, 0], base.scores[:, col]) and int(alone.iterations[0]) == int(base.iterations[col])
        assert torch.equal(alone.residual[0], base.residual[col])


# ---- 5. ranking

def _rank_rows(scores_t, dev, index_base=0):
    lib = _hip.load()
    st = torch.from_numpy(np.ascontiguousarray(scores_t)).to(dev)
    nq, n = st.shape
    need = ctypes.c_size_t()
    _hip.check(lib.gdt_retrieval_rank_scores_workspace_bytes(n, nq, ctypes.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    ranks = torch.empty((nq, n), dtype=torch.int32, device=dev)
    _hip.check(lib.gdt_retrieval_rank_scores(st.data_ptr(), ranks.data_ptr(), n, nq, index_base, ws.data_ptr(), ws.numel(),
                                             torch.cuda.current_stream(dev).cuda_stream))
    assert torch.equal(st.cpu(), torch.from_numpy(np.ascontiguousarray(scores_t)))             # the scores are left as they were
    return _np(ranks)


def test_ranks_follow_the_strict_order(cuda_device):
    shape = SOLVER_SHAPES[1]
    n, d, clusters, noise, k, kq, nq = shape
    g = _graph(n, d, clusters, noise, k)
    qv = _queries(*shape)[0]
    ranks, out = retrieval.diffusion_ranks(g["vecs"].t(), qv.t(), k=k, kq=kq, gamma=GAMMA, alpha=ALPHA, tol=TOL, max_iter=MAX_ITER,
                                           graph=(g["weights"], g["ids"]))
    assert ranks.shape == (n, nq) and ranks.dtype == torch.int32
    f = _np(out.scores)
    assert np.array_equal(_np(ranks), R.strict_ranks(f))
    # a column of zeros, both zeros in one matrix, ties and an index base
    rng = np.random.RandomState(3)
    m = rng.randint(-2, 3, (4, 257)).astype(np.float32)
    m[1] = 0
    m[2, ::3] = -0.0
    m[2, 1::3] = 0.0
    m[3, :] = np.where(rng.rand(257) < 0.5, -0.0, 0.0)
    assert np.signbit(m[2]).any() and (m[2] == 0).sum() > 100
    want = R.strict_ranks(m.T).T
    assert np.array_equal(want[1], np.arange(257)) and np.array_equal(want[3], np.arange(257))
    assert np.array_equal(_rank_rows(m, cuda_device), want)
    assert np.array_equal(_rank_rows(m, cuda_device, index_base=1000), want + 1000)
    assert np.array_equal(_np(retrieval.rank_scores(torch.from_numpy(m).to(cuda_device).t())), want.T)


# ---- 6. purpose: a query reaches the far end of its manifold through the chain of images between them

@pytest.mark.parametrize("classes,per,degrees,d,k,kq", [(8, 50, 150.0, 32, 6, 3)])
def test_diffusion_ranks_arcs_that_cosine_ranking_cannot(cuda_device, classes, per, degrees, d, k, kq):
    vecs, labels = R.arcs(0, classes, per, degrees, d, 0.01)
    gnd = R.arc_ground_truth(labels, per)
    cols = np.arange(classes) * per
    v64 = vecs.astype(np.float64)
    # the condition, from the reference alone
    cosine = retrieval.compute_map(R.strict_ranks(v64 @ v64[cols].T), gnd)[0]
    sc, ids = R.knn(vecs, k)
    Sd = R.dense(R.affinity(sc, ids, GAMMA)[1], ids)
    exact = retrieval.compute_map(R.strict_ranks(R.solve(Sd, R.seeds(*R.self_seeds(sc, ids, cols, kq, GAMMA), len(vecs)), ALPHA)), gnd)[0]
    # an AP is a sum of 1 / (2 * positives) steps, 1 up to that sum's rounding; one pair out of order costs more than 1e-4
    assert cosine < 0.7 and abs(exact - 1.0) < 1e-9, (cosine, exact)
    V = torch.from_numpy(vecs).to(cuda_device).t()
    ranks, out = retrieval.diffusion_ranks(V, None, k=k, kq=kq, gamma=GAMMA, alpha=ALPHA, tol=TOL, max_iter=MAX_ITER)
    assert ranks.shape == (len(vecs), len(vecs)) and bool((out.residual <= TOL).all())
    q_ranks = ranks[:, torch.from_numpy(cols).to(cuda_device)].contiguous()
    got = retrieval.compute_map(q_ranks, gnd)[0]
    dev_cos = retrieval.compute_map(retrieval.scores_and_ranks(V, V[:, torch.from_numpy(cols).to(cuda_device)])[1], gnd)[0]
    print("arcs: cosine mAP %.3f (device %.3f), float64 diffusion %.3f, device diffusion %.3f" % (cosine, dev_cos, exact, got))
    assert abs(got - 1.0) < 1e-9


# ---- 7. end to end

def test_diffusion_scores_equal_the_reference_pipeline_on_the_devices_lists(cuda_device):
    shape = SOLVER_SHAPES[1]
    n, d, clusters, noise, k, kq, nq = shape
    g = _graph(n, d, clusters, noise, k)
    qv, s, sid, _, _ = _queries(*shape)
    out = retrieval.diffusion_scores(g["vecs"].t(), qv.t(), k=k, kq=kq, gamma=GAMMA, alpha=ALPHA, tol=TOL, max_iter=MAX_ITER)
    # the reference pipeline in float64 throughout, from the device's kNN and top-k lists
    S64 = g["S64"]
    Sd64 = R.dense(S64, g["ids_r"])
    y64 = R.seeds(_np(sid.t()), np.power(np.maximum(_np(s.t()).astype(np.float64), 0), GAMMA), n)
    want = R.solve(Sd64, y64, ALPHA)
    f = _np(out.scores).astype(np.float64)
    ynorm = np.linalg.norm(y64, axis=0)
    true = R.true_residual(Sd64, y64, f, ALPHA)
    # against the float64 graph the device's S is off by the affinity gate per entry: |dS f| <= gate * S |f|, and the seeds by powf's 16 ulp
    slack = (AFFINITY_GATE * ALPHA * np.linalg.norm(Sd64 @ np.abs(f), axis=0) + 16 * 2.0 ** -24 * ynorm) / ynorm
    print("end to end: true residual / tol at most %.3f (slack of the graph's rounding %.2e)" % ((true / TOL).max(), slack.max()))
    assert np.all(_np(out.residual) <= TOL) and np.all(true <= 3 * TOL + slack)
    assert np.all(np.linalg.norm(f - want, axis=0) <= true * ynorm / (1 - ALPHA))
    same = retrieval.diffusion_scores(g["vecs"].t(), qv.t(), k=k, kq=kq, gamma=GAMMA, alpha=ALPHA, tol=TOL, max_iter=MAX_ITER, graph=(g["weights"], g["ids"]))
    for a, b in zip(out, same):
        assert torch.equal(a, b)
