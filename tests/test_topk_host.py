"""Streaming top-k / query expansion without a device: the oracle (tests/topk_ref.py) against a brute-force loop, and the argument checks of the C
entries and of the Python functions, all of which happen before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

import topk_ref as R
from gandtr_amd import _hip, retrieval


def _brute_topk(vecs, qvecs, k, self_base=-1):
    out = []
    for q in range(len(qvecs)):
        cand = []
        for r in range(len(vecs)):
            if self_base >= 0 and r == self_base + q:
                continue
            cand.append((-float(sum(float(a) * float(b) for a, b in zip(vecs[r], qvecs[q]))), r))
        cand.sort()
        cand = cand[:k] + [(np.inf, -1)] * (k - len(cand))
        out.append(cand)
    return np.array([[-s for s, _ in row] for row in out]), np.array([[i for _, i in row] for row in out])


def test_oracle_matches_brute_force_with_ties():
    rng = np.random.RandomState(0)
    vecs = rng.randint(-2, 3, (12, 3)).astype(np.float32)
    vecs[7] = vecs[2]                                                   # duplicated rows: ties broken by the lower row
    vecs[9] = vecs[2]
    qvecs = rng.randint(-2, 3, (4, 3)).astype(np.float32)
    for k, self_base in ((1, -1), (5, -1), (12, -1), (16, -1)):
        s, i = R.ref_topk(vecs, qvecs, k, self_base)
        bs, bi = _brute_topk(vecs, qvecs, k, self_base)
        assert np.array_equal(i, bi) and np.array_equal(s, bs)
    s, i = R.ref_topk(vecs, vecs, 4, 0)                                 # a set against itself without the diagonal
    bs, bi = _brute_topk(vecs, vecs, 4, 0)
    assert np.array_equal(i, bi) and np.array_equal(s, bs)
    assert all(q not in i[q] for q in range(12))
    q2 = np.where(i[2] == 7)[0][0]
    assert i[2][q2 + 1] == 9                                            # the duplicates of row 2, lower row first
    s, i = R.ref_topk(vecs, qvecs, 3, index_base=100)
    assert np.array_equal(i - 100, R.ref_topk(vecs, qvecs, 3)[1])


def test_oracle_expand_small_case():
    vecs = np.array([[1., 0.], [0., 1.], [1., 1.]])
    out, mag, norm = R.ref_expand(vecs, np.array([[1., 0.]]), np.array([[2, -1, 1]]), np.array([[0.5, 9., -0.3]]), 2.0)
    x = np.array([1. + 0.25, 0.25])                                     # base + 0.5^2 * (1, 1); the -1 entry and the negative score add nothing
    assert np.allclose(out[0], x / (np.linalg.norm(x) + 1e-6)) and np.allclose(mag[0], x) and np.isclose(norm[0, 0], np.linalg.norm(x))
    out, _, _ = R.ref_expand(vecs, None, np.array([[0, 1]]), np.array([[-1., -1.]]), 0.0)      # alpha 0: the plain average
    assert np.allclose(out[0], np.array([1., 1.]) / (np.sqrt(2.) + 1e-6))


def _ws(lib, ndb, nq, d, k, slices):
    need = ctypes.c_size_t()
    _hip.check(lib.gdt_retrieval_topk_workspace_bytes(ndb, nq, d, k, slices, ctypes.byref(need)))
    return need.value


def test_workspace_grows_with_slices_and_not_with_the_database():
    lib = _hip.load()
    sizes = [_ws(lib, 100000, 70, 2048, 100, s) for s in (1, 2, 7, 64, 1024)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    assert sizes[0] >= 70 * 100 * 8 and sizes[-1] <= 70 * 100 * 8 * 1024 + 70 * 1024 * 4 + 4096         # O(nq * k * slices)
    # f32-input MFMAs read the operands where they are: no copy, so no term in ndb or d at all
    assert _ws(lib, 1000, 70, 2048, 100, 7) == _ws(lib, 10 ** 9, 70, 2048, 100, 7) == _ws(lib, 1000, 70, 33, 100, 7)
    assert _ws(lib, 70000, 32768, 16, 4, 0) < (1 << 28)                 # ndb * nq beyond 2^31 is an ordinary call
    assert _ws(lib, 2 * 10 ** 5, 2 * 10 ** 5, 512, 10, 0) < (1 << 31)


@pytest.mark.parametrize("ndb,nq,d,k,slices", [(10, 2, 8, 0, 1), (10, 2, 8, 257, 1), (10, 2, 0, 4, 1), (10, 2, 8193, 4, 1), (0, 2, 8, 4, 1),
                                               (10, 0, 8, 4, 1), (10, 2, 8, 4, -1), (10, 2, 8, 4, 1025), (1 << 31, 2, 8, 4, 1)])
def test_topk_entries_refuse_bad_sizes_before_any_launch(ndb, nq, d, k, slices):
    lib = _hip.load()
    need = ctypes.c_size_t()
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_retrieval_topk_workspace_bytes(ndb, nq, d, k, slices, ctypes.byref(need)))
    one = ctypes.c_void_p(16)                                           # never dereferenced: the sizes are refused first
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_retrieval_topk(one, one, one, one, ndb, nq, d, k, 0, -1, slices, one, 1 << 20, None))
    if slices == 1 and ndb < (1 << 31):
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_retrieval_expand(one, None, one, one, one, ndb, nq, d, k, 0, 3.0, None))


def test_topk_entries_refuse_null_buffers_and_bad_bases():
    lib = _hip.load()
    one = ctypes.c_void_p(16)
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_retrieval_topk_workspace_bytes(10, 2, 8, 4, 1, None))
    for hole in range(5):
        a = [one] * 5
        a[hole] = None
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_retrieval_topk(a[0], a[1], a[2], a[3], 10, 2, 8, 4, 0, -1, 1, a[4], 1 << 20, None))
    for hole in (0, 2, 3, 4):                                           # base (argument 1) may be NULL
        a = [one] * 5
        a[hole] = None
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_retrieval_expand(a[0], a[1], a[2], a[3], a[4], 10, 2, 8, 4, 0, 3.0, None))
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_retrieval_topk(one, one, one, one, 10, 2, 8, 4, -1, -1, 1, one, 1 << 20, None))          # negative index_base
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_retrieval_topk(one, one, one, one, 10, 2, 8, 4, 2 ** 31 - 5, -1, 1, one, 1 << 20, None))  # ids past int32
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_retrieval_topk(one, one, one, one, 10, 2, 8, 4, 0, -2, 1, one, 1 << 20, None))           # self_base
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_retrieval_expand(one, None, one, one, one, 10, 2, 8, 4, 0, -1.0, None))                  # alpha
    with pytest.raises(RuntimeError, match="workspace too small"):
        _hip.check(lib.gdt_retrieval_topk(one, one, one, one, 10, 2, 8, 4, 0, -1, 1, one, 8, None))


def test_python_functions_refuse_bad_arguments():
    v, q = torch.zeros(24, 50), torch.zeros(24, 3)
    with pytest.raises(ValueError, match="one HIP device"):
        retrieval.topk(v, q, 5)
    with pytest.raises(ValueError, match="one HIP device"):
        retrieval.expand_queries(v, q, 5)
    with pytest.raises(ValueError, match="one HIP device"):
        retrieval.augment_database(v, 5)
    with pytest.raises(ValueError, match="one HIP device"):
        retrieval.knn_graph(v, 5)
    with pytest.raises(ValueError, match="descriptor sizes differ"):
        retrieval.topk(v, torch.zeros(25, 3), 5)
    with pytest.raises(ValueError, match="descriptor sizes differ"):
        retrieval.expand_queries(v, torch.zeros(25, 3), 5)
    with pytest.raises(ValueError, match="the same set"):
        retrieval.topk(v, q, 5, exclude_self=True)
    with pytest.raises(ValueError, match="the same set"):
        retrieval.topk(v, v + 1, 5, exclude_self=True)
    with pytest.raises(ValueError, match="one HIP device"):              # the same set passes that check and stops at the next one
        retrieval.topk(v, v.clone(), 5, exclude_self=True)
