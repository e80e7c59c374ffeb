"""Diffusion on the mutual kNN graph without a device: the float64 restatement (tests/diffusion_ref.py) against brute force on a hand-written graph,
the argument checks of the C entries and of the Python functions (all before anything is launched), and the conditions on the reference alone that
tests/test_hip_diffusion.py relies on."""
import ctypes

import numpy as np
import pytest
import torch

import diffusion_ref as R
from gandtr_amd import _hip, retrieval

ALPHA, TOL, MAX_ITER = 0.99, 1e-5, 64
SOLVER_SHAPES = [(300, 16, 5, 0.3, 8, 4, 5), (600, 32, 12, 0.5, 10, 5, 7), (3000, 64, 40, 0.6, 20, 10, 70)]       # n, d, clusters, noise, k, kq, nq
ARC_CASES = [(8, 50, 150.0, 32, 6, 3), (12, 40, 160.0, 64, 8, 4)]                                                 # classes, per, degrees, d, k, kq


def test_reference_matches_brute_force_on_a_hand_written_graph():
    # 0 - 1 - 2 mutual; 3 lists 0, which does not list it back; 4 is isolated (lists nobody); 5 lists 4 only (not mutual): isolated too
    ids = np.array([[1, -1, -1], [0, 2, -1], [1, -1, -1], [0, -1, -1], [-1, -1, -1], [4, 9, -1]], dtype=np.int32)      # 9: outside the database
    sc = np.array([[0.9, -np.inf, -np.inf], [0.9, 0.5, -np.inf], [0.6, -np.inf, -np.inf], [0.8, -np.inf, -np.inf], [-np.inf] * 3,
                   [0.7, 0.7, -np.inf]])
    gamma = 2.0
    w, S, deg = R.affinity(sc, ids, gamma)
    w01, w12 = min(0.9 ** 2, 0.9 ** 2), min(0.5 ** 2, 0.6 ** 2)                                 # the weaker direction of each mutual pair
    want_w = np.zeros((6, 3))
    want_w[0, 0], want_w[1, 0], want_w[1, 1], want_w[2, 0] = w01, w01, w12, w12
    assert np.array_equal(w, want_w)
    want_deg = np.array([w01, w01 + w12, w12, 0, 0, 0])
    assert np.allclose(deg, want_deg, rtol=1e-15)
    A = np.zeros((6, 6))
    A[0, 1] = A[1, 0] = w01 / np.sqrt(want_deg[0] * want_deg[1])
    A[1, 2] = A[2, 1] = w12 / np.sqrt(want_deg[1] * want_deg[2])
    Sd = R.dense(S, ids)
    assert np.allclose(Sd, A, rtol=1e-14, atol=0) and np.array_equal(Sd, Sd.T)
    assert not Sd[3:].any() and not Sd[:, 3:].any()                                              # the non-mutual edge and the isolated rows
    # seeds: a duplicate id adds, an id outside the database adds nothing, a column without a valid seed is 0
    y = R.seeds(np.array([[0, 0, 7], [4, -1, -1], [-1, 6, -1]]), np.array([[1.0, 0.5, 3.0], [2.0, 1.0, 1.0], [1.0, 1.0, 1.0]]), 6)
    assert np.array_equal(y[:, 0], [1.5, 0, 0, 0, 0, 0]) and np.array_equal(y[:, 1], [0, 0, 0, 0, 2.0, 0]) and not y[:, 2].any()
    f = R.solve(Sd, y, ALPHA)
    # brute force: the Neumann series sum_t (alpha S)^t y
    g, term = np.zeros_like(y), y.copy()
    for _ in range(6000):
        g += term
        term = ALPHA * (Sd @ term)
    assert np.allclose(f, g, rtol=1e-9, atol=1e-12)
    assert np.array_equal(f[:, 1], [0, 0, 0, 0, 2.0, 0]) and not f[:, 2].any()                   # an isolated node keeps its seed and spreads nothing
    fc, its, res = R.cg(Sd, y, ALPHA, 1e-12, 50)
    assert np.allclose(fc, f, rtol=1e-9, atol=1e-12) and its[2] == 0 and res[2] == 0 and its[1] == 1 and its[0] <= 3
    assert np.all(R.true_residual(Sd, y, fc, ALPHA) <= 1e-11)
    _, its1, res1 = R.cg(Sd, y, ALPHA, 1e-12, 1)
    assert its1[0] == 1 and res1[0] > 1e-12
    assert np.array_equal(R.strict_ranks(np.array([[0.0, 1.0], [-0.0, 1.0], [2.0, -1.0]])), [[2, 0], [0, 1], [1, 2]])


# ---- argument checks of the C entries: before any HIP call

ONE = ctypes.c_void_p(16)                                                # never dereferenced: the arguments are refused first


def _diffuse(lib, n=10, k=4, nq=2, kq=3, block=64, alpha=0.99, tol=1e-5, max_iter=64, ws_bytes=1 << 30, bufs=None):
    b = bufs or [ONE] * 8
    return lib.gdt_retrieval_diffuse(b[0], b[1], b[2], b[3], b[4], b[5], b[6], n, k, nq, kq, block, alpha, tol, max_iter, b[7], ws_bytes, None)


@pytest.mark.parametrize("bad", [dict(n=0), dict(nq=0), dict(k=0), dict(k=257), dict(kq=0), dict(kq=257), dict(block=0), dict(block=65), dict(alpha=0.0),
                                 dict(alpha=1.0), dict(alpha=-0.5), dict(tol=0.0), dict(tol=-1.0), dict(max_iter=0), dict(max_iter=1001)])
def test_diffuse_refuses_bad_sizes_before_any_launch(bad):
    lib = _hip.load()
    with pytest.raises(ValueError):
        _hip.check(_diffuse(lib, **bad))
    need = ctypes.c_size_t()
    if set(bad) & {"n", "nq", "block"}:
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_retrieval_diffuse_workspace_bytes(bad.get("n", 10), bad.get("nq", 2), bad.get("block", 64), ctypes.byref(need)))


def test_diffuse_workspace_and_null_buffers():
    lib = _hip.load()
    need = ctypes.c_size_t()
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_retrieval_diffuse_workspace_bytes(10, 2, 64, None))
    _hip.check(lib.gdt_retrieval_diffuse_workspace_bytes(200000, 70, 64, ctypes.byref(need)))
    assert 4 * 200000 * 64 * 4 <= need.value <= 4 * 200000 * 64 * 4 + (1 << 22)               # four [n][64] fp32 vectors and the partial sums
    big = need.value
    _hip.check(lib.gdt_retrieval_diffuse_workspace_bytes(200000, 70, 7, ctypes.byref(need)))
    assert need.value < big / 7                                                                # [n][8]
    _hip.check(lib.gdt_retrieval_diffuse_workspace_bytes(200000, 3, 64, ctypes.byref(need)))
    assert need.value < big / 15                                                               # no wider than the queries: [n][4]
    for hole in range(8):
        bufs = [ONE] * 8
        bufs[hole] = None
        with pytest.raises(ValueError):
            _hip.check(_diffuse(lib, bufs=bufs))
    with pytest.raises(RuntimeError, match="workspace too small"):
        _hip.check(_diffuse(lib, ws_bytes=8))


def test_affinity_and_rank_scores_refuse_bad_arguments_before_any_launch():
    lib = _hip.load()
    two = ctypes.c_void_p(32)
    for n, k, gamma in ((0, 4, 3.0), (10, 0, 3.0), (10, 257, 3.0), (10, 4, -1.0)):
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_retrieval_knn_affinity(ONE, ONE, two, ONE, n, k, gamma, None))
    for hole in range(4):
        bufs = [ONE, ONE, two, ONE]
        bufs[hole] = None
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_retrieval_knn_affinity(bufs[0], bufs[1], bufs[2], bufs[3], 10, 4, 3.0, None))
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_retrieval_knn_affinity(ONE, ONE, ONE, ONE, 10, 4, 3.0, None))         # weights on top of scores
    need = ctypes.c_size_t()
    for n, nq in ((0, 2), (10, 0), (1 << 16, 1 << 15)):                                          # the last: n * nq = 2^31
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_retrieval_rank_scores_workspace_bytes(n, nq, ctypes.byref(need)))
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_retrieval_rank_scores(ONE, ONE, n, nq, 0, ONE, 1 << 30, None))
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_retrieval_rank_scores_workspace_bytes(10, 2, None))
    for hole in range(3):
        bufs = [ONE] * 3
        bufs[hole] = None
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_retrieval_rank_scores(bufs[0], bufs[1], 10, 2, 0, bufs[2], 1 << 30, None))
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_retrieval_rank_scores(ONE, ONE, 10, 2, -1, ONE, 1 << 30, None))       # negative index_base
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_retrieval_rank_scores(ONE, ONE, 10, 2, 2 ** 31 - 5, ONE, 1 << 30, None))   # ids past int32


def test_python_functions_refuse_cpu_tensors_and_mismatched_shapes():
    s, i = torch.zeros(4, 50), torch.zeros(4, 50, dtype=torch.int32)
    with pytest.raises(ValueError, match="one HIP device"):
        retrieval.mutual_knn_affinity(s, i)
    with pytest.raises(ValueError, match="one HIP device"):
        retrieval.diffuse(s, i, torch.zeros(3, 2, dtype=torch.int32), torch.zeros(3, 2))
    with pytest.raises(ValueError, match="one HIP device"):
        retrieval.diffusion_scores(torch.zeros(16, 50))
    with pytest.raises(ValueError, match="one HIP device"):
        retrieval.diffusion_ranks(torch.zeros(16, 50), torch.zeros(16, 3))
    with pytest.raises(ValueError, match="one HIP device"):
        retrieval.rank_scores(torch.zeros(50, 3))
    with pytest.raises(ValueError, match="one shape"):
        retrieval.mutual_knn_affinity(s, torch.zeros(5, 50, dtype=torch.int32))
    with pytest.raises(ValueError, match="one shape"):
        retrieval.diffuse(s, torch.zeros(4, 51, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int32), torch.zeros(3, 2))
    with pytest.raises(ValueError, match="one shape"):
        retrieval.diffuse(s, i, torch.zeros(3, 2, dtype=torch.int32), torch.zeros(3, 3))
    with pytest.raises(ValueError, match="one shape"):
        retrieval.mutual_knn_affinity(torch.zeros(50), torch.zeros(50, dtype=torch.int32))
    with pytest.raises(ValueError, match="Ndb x Nq"):
        retrieval.rank_scores(torch.zeros(50))


# ---- the conditions on the reference alone that the GPU tests rely on

@pytest.mark.parametrize("n,d,clusters,noise,k,kq,nq", SOLVER_SHAPES)
def test_float64_cg_reaches_tol_within_half_of_max_iter(n, d, clusters, noise, k, kq, nq):
    vecs = R.clustered(n, n, d, clusters, noise)
    sc, ids = R.knn(vecs, k)
    _, S, _ = R.affinity(sc, ids, 3.0)
    Sd = R.dense(S, ids)
    assert np.array_equal(Sd, Sd.T)
    qv = R.clustered(n + 1, nq, d, clusters, noise)
    qs = qv.astype(np.float64) @ vecs.astype(np.float64).T
    sid = np.argsort(-qs, axis=1, kind="stable")[:, :kq]
    y = R.seeds(sid, np.power(np.maximum(np.take_along_axis(qs, sid, axis=1), 0), 3.0), n)
    f, its, res = R.cg(Sd, y, ALPHA, TOL, MAX_ITER)
    print("float64 CG n=%d: iterations %d .. %d" % (n, its.min(), its.max()))
    assert its.max() <= MAX_ITER // 2 and np.all(res <= TOL)
    tr = R.true_residual(Sd, y, f, ALPHA)
    assert np.all(tr <= 1.001 * TOL)
    err = np.linalg.norm(f - R.solve(Sd, y, ALPHA), axis=0)
    assert np.all(err <= tr * np.linalg.norm(y, axis=0) / (1 - ALPHA) * (1 + 1e-9))                # lambda_min(I - alpha S) >= 1 - alpha


@pytest.mark.parametrize("classes,per,degrees,d,k,kq", ARC_CASES)
def test_arcs_defeat_cosine_ranking_and_not_diffusion(classes, per, degrees, d, k, kq):
    vecs, labels = R.arcs(0, classes, per, degrees, d, 0.01)
    gnd = R.arc_ground_truth(labels, per)
    cols = np.arange(classes) * per
    v64 = vecs.astype(np.float64)
    cosine = retrieval.compute_map(R.strict_ranks(v64 @ v64[cols].T), gnd)[0]
    sc, ids = R.knn(vecs, k)
    _, S, _ = R.affinity(sc, ids, 3.0)
    Sd = R.dense(S, ids)
    y = R.seeds(*R.self_seeds(sc, ids, cols, kq, 3.0), len(vecs))
    exact = retrieval.compute_map(R.strict_ranks(R.solve(Sd, y, ALPHA)), gnd)[0]
    by_cg = retrieval.compute_map(R.strict_ranks(R.cg(Sd, y, ALPHA, TOL, MAX_ITER)[0]), gnd)[0]
    print("arcs %d x %d: cosine mAP %.3f, diffusion %.3f (CG %.3f)" % (classes, per, cosine, exact, by_cg))
    # an AP is a sum of 1 / (2 * positives) steps, 1 up to that sum's rounding; one pair out of order costs more than 1e-4
    assert cosine < 0.7 and abs(exact - 1.0) < 1e-9 and abs(by_cg - 1.0) < 1e-9
