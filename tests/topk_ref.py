"""numpy float64 oracle of the streaming top-k and of the weighted expansion (gandtr_amd/csrc/retrieval_topk.hip).  The formulas here are the
specification.  Row conventions of the C ABI: vecs [ndb][d], qvecs [nq][d], results [nq][k]."""
import numpy as np


def ref_scores(vecs, qvecs):
    """float64 inner products [nq][ndb]"""
    return np.dot(np.asarray(qvecs, dtype=np.float64), np.asarray(vecs, dtype=np.float64).T)


def ref_topk(vecs, qvecs, k, self_base=-1, index_base=0):
    """per query the first k rows in the strict order (score descending, row ascending): (scores [nq][k] float64, ids [nq][k] int64);
    with fewer than k rows the tail is id -1, score -inf.  self_base >= 0 leaves row self_base + q out for query q."""
    s = ref_scores(vecs, qvecs)
    nq, ndb = s.shape
    out_s = np.full((nq, k), -np.inf)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    rows = np.arange(ndb)
    for q in range(nq):
        keep = rows if self_base < 0 else rows[rows != self_base + q]
        order = keep[np.lexsort((keep, -s[q, keep]))[:k]]
        out_s[q, :len(order)] = s[q, order]
        out_i[q, :len(order)] = order + index_base
    return out_s, out_i


def expand_weights(scores, alpha):
    scores = np.asarray(scores, dtype=np.float64)
    return np.ones_like(scores) if alpha == 0 else np.maximum(scores, 0.0) ** alpha


def ref_expand(vecs, base, ids, scores, alpha, index_base=0):
    """x = (base or 0) + sum_{ids >= 0} w_j vecs[ids_j - index_base];  returns (x / (||x|| + 1e-6), magnitude) in float64, where magnitude
    [nq][d] = |base_i| + sum_j |w_j v_ji| is the quantity the rounding bound of the fp32 sum scales with."""
    vecs = np.asarray(vecs, dtype=np.float64)
    ids = np.asarray(ids)
    w = expand_weights(scores, alpha)
    nq, k = ids.shape
    x = np.zeros((nq, vecs.shape[1])) if base is None else np.asarray(base, dtype=np.float64).copy()
    mag = np.abs(x)
    for q in range(nq):
        for j in range(k):
            if ids[q, j] >= 0:
                term = w[q, j] * vecs[ids[q, j] - index_base]
                x[q] += term
                mag[q] += np.abs(term)
    norm = np.sqrt((x * x).sum(axis=1, keepdims=True))
    return x / (norm + 1e-6), mag, norm
