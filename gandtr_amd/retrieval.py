"""Retrieval scoring on the device -- the consumer of the gathered descriptors.

Reference (CPU numpy): ``scores = np.dot(vecs.T, qvecs); ranks = np.argsort(-scores, axis=0)``
(mdir/components/optim/score/cirscore.py:71-73); hard-negative mining does the same with torch.mm / torch.sort
(mdir/external/cirtorch/datasets/traindataset.py:246-279).  Same layout conventions here: descriptors are D x N (one column
per image, views of the library's [N][D] blocks), scores are Ndb x Nq, ranks are Ndb x Nq database indices per query column.
"""
import collections
import ctypes

import numpy as np
import torch
import torch.distributed as dist

from . import _hip


def _rows(m):
    """D x N (any strides) -> contiguous [N][D] fp32"""
    return m.t().contiguous().float()


def scores_and_ranks(vecs, qvecs, with_ranks=True, index_base=0):
    """vecs: D x Ndb, qvecs: D x Nq (cuda).  Returns (scores Ndb x Nq fp32, ranks Ndb x Nq int32 or None)."""
    lib = _hip.load()
    if not vecs.is_cuda or vecs.device != qvecs.device:
        raise ValueError("scores_and_ranks needs descriptors on one HIP device")
    v, q = _rows(vecs), _rows(qvecs)
    ndb, d = v.shape
    nq = q.shape[0]
    if q.shape[1] != d:
        raise ValueError("descriptor sizes differ: %d vs %d" % (d, q.shape[1]))
    need = ctypes.c_size_t()
    with torch.cuda.device(v.device):
        _hip.check(lib.gdt_retrieval_workspace_bytes(ndb, nq, d, int(with_ranks), ctypes.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=v.device)
        scores_t = torch.empty((nq, ndb), dtype=torch.float32, device=v.device)
        ranks_t = torch.empty((nq, ndb), dtype=torch.int32, device=v.device) if with_ranks else None
        _hip.check(lib.gdt_retrieval_scores_ranks(v.data_ptr(), q.data_ptr(), scores_t.data_ptr(),
                                                  ranks_t.data_ptr() if with_ranks else None, ndb, nq, d, index_base,
                                                  ws.data_ptr(), ws.numel(), torch.cuda.current_stream(v.device).cuda_stream))
    return scores_t.t(), (ranks_t.t() if with_ranks else None)


def select_negatives(ranks, pool_clusters, query_clusters, vecs, qvecs, nnum, index_base=0):
    """The selection loop of the reference's hard-negative mining on the device (traindataset.py:256-275): per query (column of ``ranks``,
    Ndb x Nq as returned by ``scores_and_ranks``) the first ``nnum`` pool positions whose cluster is neither the query's nor that of a
    position already taken.  pool_clusters: Ndb ints, query_clusters: Nq ints.  Returns (positions Nq x nnum int32, distances Nq x nnum fp32 =
    ||q - p + 1e-6||_2, the reference's statistic).  Raises IndexError where the reference's ``ranks[r, q]`` would run past the pool."""
    lib = _hip.load()
    dev = vecs.device
    v, q = _rows(vecs), _rows(qvecs)
    ndb, d = v.shape
    nq = q.shape[0]
    rk = ranks.t().contiguous().to(torch.int32)                               # [Nq][Ndb]
    pc = torch.as_tensor(pool_clusters, dtype=torch.int32, device=dev).contiguous()
    qc = torch.as_tensor(query_clusters, dtype=torch.int32, device=dev).contiguous()
    if rk.shape != (nq, ndb) or pc.numel() != ndb or qc.numel() != nq:
        raise ValueError("ranks is Ndb x Nq, pool_clusters has Ndb and query_clusters Nq entries")
    pos = torch.empty((nq, nnum), dtype=torch.int32, device=dev)
    dist_ = torch.empty((nq, nnum), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _hip.check(lib.gdt_retrieval_select_negatives(rk.data_ptr(), pc.data_ptr(), qc.data_ptr(), v.data_ptr(), q.data_ptr(), pos.data_ptr(),
                                                      dist_.data_ptr(), status.data_ptr(), ndb, nq, d, int(nnum), int(index_base),
                                                      torch.cuda.current_stream(dev).cuda_stream))
    if int(status.item()) & 1:
        raise IndexError("hard-negative selection ran past the pool: fewer than %d other clusters among its images" % nnum)
    return pos, dist_


def search_hard_negatives(qidxs, qvecs, idxs2images, poolvecs, clusters, nnum):
    """``TuplesDataset._search_hard_negatives`` (traindataset.py:246-279) with scores, sort AND the cluster-aware selection on the device.
    qidxs: image index per query; qvecs: D x Nq; idxs2images: image index per pool position; poolvecs: D x Npool; clusters: cluster id per image
    index (``self.clusters``); nnum negatives per query.  Returns what the reference returns: (nidxs -- a list of nnum image indices per query --,
    {"average_negative_distance": [one l2 distance per chosen negative, query by query]})."""
    clusters = torch.as_tensor(clusters)
    idxs2images_t = torch.as_tensor(idxs2images, dtype=torch.int64)
    _, ranks = scores_and_ranks(poolvecs, qvecs)
    pos, dist_ = select_negatives(ranks, clusters[idxs2images_t], clusters[torch.as_tensor(qidxs, dtype=torch.int64)], poolvecs, qvecs, nnum)
    nidxs = idxs2images_t[pos.cpu().long()].tolist()
    return nidxs, {"average_negative_distance": dist_.cpu().reshape(-1).tolist()}


# ---- diverse-anchor selection (mdir/components/data/dataset/cirtorch_datasets.py:77-100)

def diverse_anchor_targets(qpool_size, qsize, similar_exclude, similar_include, shuffle):
    """The position in the ascending order of ``most_similar`` that every step of the reference's loop picks (cirtorch_datasets.py:88-95),
    evaluated up front: int64 [qsize-1].  The slice ``argsort()[dissimilar_split:similar_split]`` depends on the step number alone, so with
    ``shuffle`` the ``torch.randint(slice size, (1,))`` draws happen here, one per step in step order -- the global generator is consumed
    exactly as by the reference's loop, which draws nothing else."""
    targets = torch.empty(max(qsize - 1, 0), dtype=torch.int64)
    for t in range(qsize - 1):
        valid_size = qpool_size - (t + 1)
        similar_split = max(int(valid_size * (1 - similar_exclude)), 1)
        dissimilar_split = min(int(valid_size * (1 - similar_include)), similar_split - 1)
        size = similar_split - dissimilar_split
        choice = torch.randint(size, (1,)).item() if shuffle else size - 1
        targets[t] = dissimilar_split + choice
    return targets


def diverse_anchors(qvecs, target_rank, first_idx=0):
    """The chain of ``gdt_retrieval_diverse_anchors`` on explicit targets.  qvecs: D x Q fp32 on a HIP device (any strides); target_rank:
    host integers, one per step, each in [0, Q) -- checked here, before anything is launched.  Returns (idxs int32 [len + 1], scores fp32
    [len]) on the device, enqueued on the current stream without a synchronisation.  Equal similarities rank by lower index first."""
    lib = _hip.load()
    if not torch.is_tensor(qvecs) or not qvecs.is_cuda:
        raise ValueError("diverse_anchors needs the descriptors on a HIP device")
    v = _rows(qvecs)
    nq, d = v.shape
    tr = torch.as_tensor(target_rank, dtype=torch.int64).reshape(-1).cpu()
    nsel = tr.numel() + 1
    if nsel < 2 or nsel > nq:
        raise ValueError("between 1 and %d steps for %d descriptors, got %d" % (nq - 1, nq, nsel - 1))
    if int(tr.min()) < 0 or int(tr.max()) >= nq:
        raise ValueError("target_rank outside [0, %d)" % nq)
    dev = v.device
    need = ctypes.c_size_t()
    with torch.cuda.device(dev):
        _hip.check(lib.gdt_retrieval_diverse_anchors_workspace_bytes(nq, d, nsel, ctypes.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        d_tr = tr.to(torch.int32).to(dev)
        idxs = torch.empty(nsel, dtype=torch.int32, device=dev)
        scores = torch.empty(nsel - 1, dtype=torch.float32, device=dev)
        _hip.check(lib.gdt_retrieval_diverse_anchors(v.data_ptr(), nq, d, d_tr.data_ptr(), nsel, int(first_idx), idxs.data_ptr(), scores.data_ptr(),
                                                     ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
    return idxs, scores


def _diverse_anchors_host(qvecs, targets):
    """the reference's loop on a running maximum instead of the growing ``cat`` (the same values); ties by lower index"""
    idx, idxs, qscore_acc = 0, [0], []
    most_similar = torch.full((qvecs.shape[1],), -float("inf"), dtype=qvecs.dtype)
    for target in targets.tolist():
        most_similar = torch.maximum(most_similar, torch.mm(qvecs.t(), qvecs[:, idx:idx + 1])[:, 0])
        idx = most_similar.argsort(stable=True)[target].item()
        qscore_acc.append(most_similar[idx].item())
        idxs.append(idx)
    return idxs, qscore_acc


def select_diverse_anchors(qvecs, qsize, similar_exclude, similar_include, shuffle=True):
    """The diverse-anchor selection of ``DiverseAnchorsDataset._select_positive_pairs_db`` (cirtorch_datasets.py:77-100).  qvecs: D x Q
    descriptors of the query pool.  Starting from column 0, every step keeps the largest similarity of each column to the anchors picked
    so far and takes the column at a position of that ascending order inside [dissimilar_split, similar_split) -- the last one, or with
    ``shuffle`` a random one (``diverse_anchor_targets``).  A HIP tensor runs the device chain (``diverse_anchors``), a CPU tensor the
    torch restatement.  Returns (idxs: qsize columns, qscore_acc: the qsize-1 similarities at which they were picked).  Columns already
    picked are not excluded, as in the reference; where two similarities are equal the lower column comes first (the reference's
    ``argsort`` leaves that order open)."""
    assert similar_exclude <= similar_include
    nq = qvecs.shape[1]
    if qsize < 2 or qsize > nq:
        raise ValueError("2 <= qsize <= %d descriptors, got %d" % (nq, qsize))
    targets = diverse_anchor_targets(nq, qsize, similar_exclude, similar_include, shuffle)
    if int(targets.min()) < 0 or int(targets.max()) >= nq:
        raise ValueError("similar_exclude / similar_include put a target outside [0, %d)" % nq)
    with torch.no_grad():
        if qvecs.is_cuda:
            idxs, scores = diverse_anchors(qvecs, targets)
            return idxs.cpu().tolist(), scores.cpu().tolist()
        return _diverse_anchors_host(qvecs, targets)


def sharded_topk(vecs_local, qvecs, k, group=None):
    """Database sharded over the ranks of one node (contiguous chunks, as gandtr_amd.sharding), queries replicated.
    Every rank scores its shard, keeps its local top-k per query and all-gathers the candidates (k scores + k global ids per
    query and rank: tiny, latency-bound); the final order is the top-k of the world*k candidates.
    Returns (scores k x Nq, ids k x Nq) identical on every rank."""
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    n_local = torch.tensor([vecs_local.shape[1]], device=vecs_local.device, dtype=torch.int64)
    counts = [torch.zeros_like(n_local) for _ in range(world)]
    dist.all_gather(counts, n_local, group=group)
    base = int(sum(int(c.item()) for c in counts[:rank]))
    nq = qvecs.shape[1]
    kk = min(k, max(int(c.item()) for c in counts))
    cand_s = torch.full((nq, kk), -float("inf"), dtype=torch.float32, device=qvecs.device)
    cand_i = torch.full((nq, kk), -1, dtype=torch.int32, device=qvecs.device)
    if vecs_local.shape[1] > 0:
        scores, ranks = scores_and_ranks(vecs_local, qvecs, True, index_base=base)
        top = min(kk, vecs_local.shape[1])
        ids = ranks.t()[:, :top].contiguous()                                  # nq x top, global ids
        cand_i[:, :top] = ids
        cand_s[:, :top] = torch.gather(scores.t(), 1, (ids - base).long())
    all_s = torch.empty((world * nq, kk), dtype=torch.float32, device=qvecs.device)      # rank blocks stacked along dim 0
    all_i = torch.empty((world * nq, kk), dtype=torch.int32, device=qvecs.device)
    dist.all_gather_into_tensor(all_s, cand_s, group=group)
    dist.all_gather_into_tensor(all_i, cand_i, group=group)
    flat_s = all_s.view(world, nq, kk).permute(1, 0, 2).reshape(nq, world * kk)
    flat_i = all_i.view(world, nq, kk).permute(1, 0, 2).reshape(nq, world * kk)
    order = torch.argsort(flat_s, dim=1, descending=True, stable=True)[:, :k]   # world*k candidates per query: bookkeeping
    return torch.gather(flat_s, 1, order).t(), torch.gather(flat_i, 1, order.long()).t()


# ---- streaming top-k, query expansion and database augmentation (gandtr_amd/csrc/retrieval_topk.hip)

def _on_one_device(name, *tensors):
    if not all(torch.is_tensor(t) and t.is_cuda for t in tensors) or any(t.device != tensors[0].device for t in tensors):
        raise ValueError("%s needs descriptors on one HIP device" % name)


def _topk_rows(v, q, k, index_base=0, self_base=-1, slices=0):
    """gdt_retrieval_topk on contiguous fp32 rows: v [Ndb][D], q [Nq][D] -> (scores [Nq][k] fp32, ids [Nq][k] int32).  slices = 0: the library's choice."""
    lib = _hip.load()
    ndb, d = v.shape
    nq = q.shape[0]
    need = ctypes.c_size_t()
    _hip.check(lib.gdt_retrieval_topk_workspace_bytes(ndb, nq, d, int(k), int(slices), ctypes.byref(need)))
    with torch.cuda.device(v.device):
        ws = torch.empty(need.value, dtype=torch.uint8, device=v.device)
        scores = torch.empty((nq, int(k)), dtype=torch.float32, device=v.device)
        ids = torch.empty((nq, int(k)), dtype=torch.int32, device=v.device)
        _hip.check(lib.gdt_retrieval_topk(v.data_ptr(), q.data_ptr(), ids.data_ptr(), scores.data_ptr(), ndb, nq, d, int(k), int(index_base),
                                          int(self_base), int(slices), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(v.device).cuda_stream))
    return scores, ids


def _expand_rows(v, base, ids, scores, alpha, index_base=0):
    """gdt_retrieval_expand on contiguous rows: v [Ndb][D], base [Nq][D] or None, ids / scores [Nq][k] -> [Nq][D] unit rows."""
    lib = _hip.load()
    ndb, d = v.shape
    nq, k = ids.shape
    ids, scores = ids.contiguous(), scores.contiguous()
    with torch.cuda.device(v.device):
        out = torch.empty((nq, d), dtype=torch.float32, device=v.device)
        _hip.check(lib.gdt_retrieval_expand(v.data_ptr(), base.data_ptr() if base is not None else None, ids.data_ptr(), scores.data_ptr(),
                                            out.data_ptr(), ndb, nq, d, k, int(index_base), float(alpha),
                                            torch.cuda.current_stream(v.device).cuda_stream))
    return out


def _same_set(vecs, qvecs):
    if vecs is qvecs:
        return True
    return vecs.shape == qvecs.shape and vecs.device == qvecs.device and bool(torch.equal(vecs, qvecs))


def topk(vecs, qvecs, k, index_base=0, exclude_self=False):
    """Per query the k best database entries without the Ndb x Nq score matrix.  vecs: D x Ndb, qvecs: D x Nq (one HIP device), any D up to
    8192, no limit on Ndb * Nq, 1 <= k <= 256.  Returns (scores k x Nq fp32, ids k x Nq int32 = index_base + database column), per column in the
    strict order (score descending, id ascending); with Ndb < k the tail is id -1 / score -inf.  ``exclude_self`` (vecs and qvecs are the same
    set) leaves column j out of the answer for query j."""
    if vecs.shape[0] != qvecs.shape[0]:
        raise ValueError("descriptor sizes differ: %d vs %d" % (vecs.shape[0], qvecs.shape[0]))
    if exclude_self and not _same_set(vecs, qvecs):
        raise ValueError("exclude_self needs vecs and qvecs to be the same set")
    _on_one_device("topk", vecs, qvecs)
    v = _rows(vecs)
    scores, ids = _topk_rows(v, v if vecs is qvecs else _rows(qvecs), k, index_base, 0 if exclude_self else -1)
    return scores.t(), ids.t()


def expand_queries(vecs, qvecs, k, alpha=3.0):
    """alpha-weighted query expansion: every query becomes the renormalised sum of itself and its k best database vectors, each weighted by
    max(score, 0) ** alpha (alpha = 0: the plain average, AQE).  vecs: D x Ndb, qvecs: D x Nq -> D x Nq unit columns."""
    if vecs.shape[0] != qvecs.shape[0]:
        raise ValueError("descriptor sizes differ: %d vs %d" % (vecs.shape[0], qvecs.shape[0]))
    _on_one_device("expand_queries", vecs, qvecs)
    v, q = _rows(vecs), _rows(qvecs)
    scores, ids = _topk_rows(v, q, k)
    return _expand_rows(v, q, ids, scores, alpha).t()


def augment_database(vecs, k, alpha=3.0, block=8192):
    """Database-side augmentation: every database vector becomes the weighted, renormalised sum of its own k best matches in the database
    (itself among them, found by the search).  vecs: D x Ndb -> D x Ndb unit columns.  Runs in blocks of ``block`` query columns, so memory
    stays O(Ndb * D + block * k); the block size does not show in the result."""
    _on_one_device("augment_database", vecs)
    if block < 1:
        raise ValueError("block >= 1")
    v = _rows(vecs)
    out = torch.empty_like(v)
    for b0 in range(0, v.shape[0], int(block)):
        q = v[b0:b0 + int(block)]
        scores, ids = _topk_rows(v, q, k)
        out[b0:b0 + q.shape[0]] = _expand_rows(v, None, ids, scores, alpha)
    return out.t()


def knn_graph(vecs, k, block=8192):
    """Each vector's k best neighbours other than itself: (scores k x N fp32, ids k x N int32).  ``topk`` with ``exclude_self`` in blocks of
    ``block`` query columns."""
    _on_one_device("knn_graph", vecs)
    if block < 1:
        raise ValueError("block >= 1")
    v = _rows(vecs)
    n = v.shape[0]
    scores = torch.empty((n, int(k)), dtype=torch.float32, device=v.device)
    ids = torch.empty((n, int(k)), dtype=torch.int32, device=v.device)
    for b0 in range(0, n, int(block)):
        q = v[b0:b0 + int(block)]
        scores[b0:b0 + q.shape[0]], ids[b0:b0 + q.shape[0]] = _topk_rows(v, q, k, 0, b0)
    return scores.t(), ids.t()


# ---- diffusion re-ranking on the mutual kNN graph (gandtr_amd/csrc/retrieval_diffusion.hip; Iscen et al., CVPR 2017)

DiffusionResult = collections.namedtuple("DiffusionResult", ["scores", "iterations", "residual"])
DiffusionResult.__doc__ = """scores N x Nq fp32 (a view of the library's [Nq][N] block), iterations int32 [Nq], residual fp32 [Nq]: the final relative
residual ||r|| / ||y|| of the conjugate-gradient recurrence per column (above ``tol`` where ``max_iter`` ended the column)."""


def _lists(name, a, b, dtype_b):
    """two k x N lists on one HIP device -> contiguous [N][k] rows"""
    if not (torch.is_tensor(a) and torch.is_tensor(b)) or a.dim() != 2 or a.shape != b.shape:
        raise ValueError("%s: the two lists have one shape (k x N)" % name)
    _on_one_device(name, a, b)
    return a.t().contiguous().float(), b.t().contiguous().to(dtype_b)


def mutual_knn_affinity(scores, ids, gamma=3.0):
    """Normalised weights of the mutual kNN graph.  scores / ids: k x N as ``knn_graph`` returns them.  Edge (i, s) with j = ids[s, i] keeps
    min(max(score, 0) ** gamma of i -> j, the same of j -> i) where j lists i too, else 0; the weights are scaled by 1 / sqrt(degree) on both
    ends (isolated rows stay 0).  Returns weights k x N fp32 for the same ``ids``: symmetric bit for bit."""
    lib = _hip.load()
    sc, idx = _lists("mutual_knn_affinity", scores, ids, torch.int32)
    n, k = sc.shape
    with torch.cuda.device(sc.device):
        w = torch.empty_like(sc)
        rnorm = torch.empty(n, dtype=torch.float32, device=sc.device)
        _hip.check(lib.gdt_retrieval_knn_affinity(idx.data_ptr(), sc.data_ptr(), w.data_ptr(), rnorm.data_ptr(), n, k, float(gamma),
                                                  torch.cuda.current_stream(sc.device).cuda_stream))
    return w.t()


def diffuse(weights, ids, seed_ids, seed_weights, alpha=0.99, tol=1e-5, max_iter=64, block=64):
    """Solves (I - alpha S) f = y for every query column by conjugate gradients on the device.  weights / ids: k x N (``mutual_knn_affinity``
    and the ids it was given); seed_ids / seed_weights: kq x Nq, y[seed_ids[t, q], q] += seed_weights[t, q] (duplicates add, ids outside
    [0, N) add nothing).  ``block`` columns (1 .. 64) are solved together; it does not show in the result.  Returns ``DiffusionResult``."""
    lib = _hip.load()
    if not (torch.is_tensor(seed_ids) and torch.is_tensor(seed_weights)) or seed_ids.dim() != 2 or seed_ids.shape != seed_weights.shape:
        raise ValueError("diffuse: seed_ids and seed_weights have one shape (kq x Nq)")
    w, idx = _lists("diffuse", weights, ids, torch.int32)
    sw, sid = _lists("diffuse", seed_weights, seed_ids, torch.int32)
    if sw.device != w.device:
        raise ValueError("diffuse needs descriptors on one HIP device")
    (n, k), (nq, kq), dev = w.shape, sw.shape, w.device
    need = ctypes.c_size_t()
    _hip.check(lib.gdt_retrieval_diffuse_workspace_bytes(n, nq, int(block), ctypes.byref(need)))
    with torch.cuda.device(dev):
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        scores_t = torch.empty((nq, n), dtype=torch.float32, device=dev)
        iterations = torch.empty(nq, dtype=torch.int32, device=dev)
        residual = torch.empty(nq, dtype=torch.float32, device=dev)
        _hip.check(lib.gdt_retrieval_diffuse(idx.data_ptr(), w.data_ptr(), sid.data_ptr(), sw.data_ptr(), scores_t.data_ptr(), iterations.data_ptr(),
                                             residual.data_ptr(), n, k, nq, kq, int(block), float(alpha), float(tol), int(max_iter), ws.data_ptr(),
                                             ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
    return DiffusionResult(scores_t.t(), iterations, residual)


def diffusion_scores(vecs, qvecs=None, k=50, kq=10, gamma=3.0, alpha=0.99, tol=1e-5, max_iter=64, graph=None):
    """Diffusion scores of every database image for every query.  vecs: D x N; the graph is ``mutual_knn_affinity(*knn_graph(vecs, k), gamma)``
    unless ``graph`` = (weights, ids), both k x N, is given (one graph serves many query sets).  qvecs: D x Nq -- the seeds of a query are its
    ``topk(vecs, qvecs, kq)`` with weights max(score, 0) ** gamma.  ``qvecs=None`` is the database side: query j is database column j, seeded by
    itself with weight 1 and by the first kq entries of its own kNN row, weighted the same way (N x N scores).  Returns ``DiffusionResult``."""
    _on_one_device("diffusion_scores", vecs)
    knn = None
    if graph is None:
        knn = knn_graph(vecs, k)
        graph = (mutual_knn_affinity(knn[0], knn[1], gamma), knn[1])
    weights, ids = graph
    if qvecs is None:
        if knn is None or kq > knn[0].shape[0]:
            knn = knn_graph(vecs, kq)
        own = torch.arange(vecs.shape[1], dtype=torch.int32, device=vecs.device)[None, :]
        seed_ids = torch.cat([own, knn[1][:kq]])
        seed_w = torch.cat([torch.ones_like(own, dtype=torch.float32), knn[0][:kq].clamp_min(0).pow(gamma)])
    else:
        s, seed_ids = topk(vecs, qvecs, kq)
        seed_w = s.clamp_min(0).pow(gamma)
    return diffuse(weights, ids, seed_ids, seed_w, alpha, tol, max_iter)


def rank_scores(scores, index_base=0):
    """Ranks of a given score matrix.  scores: Ndb x Nq fp32 on a HIP device -> ranks Ndb x Nq int32, per column the database indices in the strict
    order (score descending, id ascending), -0.0 taken as 0.0: the dtype and orientation of ``scores_and_ranks``.  Ndb * Nq < 2^31."""
    lib = _hip.load()
    if not torch.is_tensor(scores) or scores.dim() != 2:
        raise ValueError("rank_scores takes an Ndb x Nq matrix")
    _on_one_device("rank_scores", scores)
    st = scores.t().contiguous().float()
    nq, n = st.shape
    need = ctypes.c_size_t()
    with torch.cuda.device(st.device):
        _hip.check(lib.gdt_retrieval_rank_scores_workspace_bytes(n, nq, ctypes.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=st.device)
        ranks_t = torch.empty((nq, n), dtype=torch.int32, device=st.device)
        _hip.check(lib.gdt_retrieval_rank_scores(st.data_ptr(), ranks_t.data_ptr(), n, nq, int(index_base), ws.data_ptr(), ws.numel(),
                                                 torch.cuda.current_stream(st.device).cuda_stream))
    return ranks_t.t()


def diffusion_ranks(vecs, qvecs=None, k=50, kq=10, gamma=3.0, alpha=0.99, tol=1e-5, max_iter=64, graph=None):
    """``diffusion_scores`` and the ranking of its scores: (ranks Ndb x Nq int32 as ``scores_and_ranks`` returns them -- ``compute_map`` takes
    them --, the ``DiffusionResult``)."""
    result = diffusion_scores(vecs, qvecs, k, kq, gamma, alpha, tol, max_iter, graph)
    return rank_scores(result.scores), result


# ---- mAP evaluation (mdir/external/cirtorch/utils/evaluate.py): average precision and precision@k per query

def _id_list(x):
    """a ground-truth id list as int64 (ids that no int32 holds cannot match a database index: -1)"""
    a = np.asarray(x).reshape(-1)
    if a.size == 0:
        return np.zeros(0, dtype=np.int64)
    if a.dtype.kind == "f":
        a = np.where(a == np.floor(a), a, -1)
    a = a.astype(np.int64)
    return np.where((a >= 0) & (a < 2 ** 31), a, -1)


def _csr(lists):
    offs = np.zeros(len(lists) + 1, dtype=np.int32)
    arrs = [_id_list(x) for x in lists]
    offs[1:] = np.cumsum([len(a) for a in arrs])
    ids = np.concatenate(arrs).astype(np.int32) if arrs else np.zeros(0, dtype=np.int32)
    return offs, ids


def average_precision(ranks, gnd_setups, kappas=()):
    """AP and precision@k of every query on the device (gandtr_amd/csrc/retrieval.hip: gdt_retrieval_average_precision).

    ranks: Ndb x Nq database indices best first (cuda; as ``scores_and_ranks`` returns them).  gnd_setups: a list of setups, each a list of
    Nq dicts ``{"ok": ids, "junk": ids}`` (a missing "junk" is an empty list), matched the way ``compute_map`` matches them (np.in1d).
    Returns (aps [nsetups][Nq], prs [nsetups][Nq][len(kappas)]) as float64 numpy arrays: ``compute_map``'s ``aps`` / ``prs`` bit for bit,
    NaN for a query without positives.  Raises ValueError where ranks is not a permutation per query, and where a query with positives
    finds none of them while kappas are asked for (the reference's ``max()`` of an empty array)."""
    lib = _hip.load()
    if not torch.is_tensor(ranks) or not ranks.is_cuda:
        raise ValueError("average_precision needs the ranks on a HIP device")
    dev = ranks.device
    ndb, nq = ranks.shape
    nsetups = len(gnd_setups)
    if nsetups < 1 or any(len(g) != nq for g in gnd_setups):
        raise ValueError("one ground-truth entry per query (%d) in every setup" % nq)
    kappas = [int(k) for k in kappas]
    ok_off, ok_ids = _csr([g[i]["ok"] for g in gnd_setups for i in range(nq)])
    junk_off, junk_ids = _csr([g[i].get("junk", []) for g in gnd_setups for i in range(nq)])
    kap = (ctypes.c_int * max(len(kappas), 1))(*kappas)
    need = ctypes.c_size_t()
    _hip.check(lib.gdt_retrieval_ap_workspace_bytes(ndb, nq, nsetups, int(ok_off[-1]), ctypes.byref(need)))
    rk = ranks.t().contiguous().to(torch.int32)                                       # [Nq][Ndb]
    dv = lambda a: torch.from_numpy(a).to(dev)                                          # noqa: E731
    d_ok_off, d_ok_ids, d_junk_off, d_junk_ids = dv(ok_off), dv(ok_ids), dv(junk_off), dv(junk_ids)
    ap = torch.empty((nsetups, nq), dtype=torch.float64, device=dev)
    prk = torch.empty((nsetups, nq, len(kappas)), dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ip = ctypes.POINTER(ctypes.c_int)
    with torch.cuda.device(dev):
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        _hip.check(lib.gdt_retrieval_average_precision(
            rk.data_ptr(), ndb, nq, nsetups, d_ok_off.data_ptr(), d_ok_ids.data_ptr() if ok_ids.size else None, d_junk_off.data_ptr(),
            d_junk_ids.data_ptr() if junk_ids.size else None, ok_off.ctypes.data_as(ip), junk_off.ctypes.data_as(ip), kap, len(kappas),
            ap.data_ptr(), prk.data_ptr() if len(kappas) else None, status.data_ptr(), ws.data_ptr(), ws.numel(),
            torch.cuda.current_stream(dev).cuda_stream))
    st = int(status.item())
    if st & 1:
        raise ValueError("ranks is not a permutation of 0..%d in every query column" % (ndb - 1))
    if st & 2:
        raise ValueError("max() arg is an empty sequence: a query with positives found none of them, precision@k is undefined")
    return ap.cpu().numpy(), prk.cpu().numpy()


def _mean_over_valid(aps, prs):
    """compute_map's reduction: in-order sum over the queries with positives, divided by their number (NaN when there are none)"""
    total, pr, n = 0., np.zeros(prs.shape[1]), 0
    for i in range(len(aps)):
        if np.isnan(aps[i]):
            continue
        total = total + aps[i]
        pr = pr + prs[i, :]
        n += 1
    if n == 0:
        return float("nan"), np.full(prs.shape[1], np.nan)
    return total / n, pr / n


def _ap_host(pos, nres):
    ap = 0
    step = 1. / nres
    for j, r in enumerate(pos):
        p0 = 1. if r == 0 else float(j) / r
        p1 = float(j + 1) / (r + 1)
        ap += (p0 + p1) * step / 2.
    return ap


def _map_host(ranks, gnd, kappas):
    """the numpy restatement of compute_map (evaluate.py:39-118): the CPU branch of ``compute_map``"""
    nq = len(gnd)
    aps = np.zeros(nq)
    prs = np.zeros((nq, len(kappas)))
    positions = np.arange(ranks.shape[0])
    for i in range(nq):
        ok = np.array(gnd[i]["ok"])
        if ok.shape[0] == 0:
            aps[i] = np.nan
            prs[i, :] = np.nan
            continue
        junk = np.array(gnd[i]["junk"]) if "junk" in gnd[i] else np.empty(0)
        pos = positions[np.isin(ranks[:, i], ok)]
        jpos = positions[np.isin(ranks[:, i], junk)]
        # a positive moves up by the number of junk images strictly before it
        pos = pos - np.searchsorted(jpos, pos, side="left")
        aps[i] = _ap_host(pos, len(ok))
        pos = pos + 1
        for j, kappa in enumerate(kappas):
            kq = min(max(pos), kappa)
            prs[i, j] = (pos <= kq).sum() / kq
    return aps, prs


def compute_map(ranks, gnd, kappas=[]):
    """``compute_map`` (evaluate.py:39-118): returns (map, aps, pr, prs).  ranks Ndb x Nq: a cuda tensor runs the device kernel
    (``average_precision``), a numpy array the host restatement; same doubles either way.  With no query that has positives, map and pr
    are NaN."""
    if torch.is_tensor(ranks) and ranks.is_cuda:
        aps, prs = average_precision(ranks, [gnd], kappas)
        aps, prs = aps[0], prs[0]
    else:
        aps, prs = _map_host(np.asarray(ranks), gnd, list(kappas))
    m, pr = _mean_over_valid(aps, prs)
    return m, aps, pr, prs


def _revisited_setups(gnd):
    """easy / medium / hard ground truth of the revisited protocol (evaluate.py:118-140)"""
    cat = lambda *xs: np.concatenate([np.asarray(x) for x in xs])                     # noqa: E731
    return [[{"ok": cat(g["easy"]), "junk": cat(g["junk"], g["hard"])} for g in gnd],
            [{"ok": cat(g["easy"], g["hard"]), "junk": cat(g["junk"])} for g in gnd],
            [{"ok": cat(g["hard"]), "junk": cat(g["junk"], g["easy"])} for g in gnd]]


def compute_map_and_print(dataset, ranks, gnd, kappas=[1, 5, 10]):
    """``compute_map_and_print`` (evaluate.py:121-155): prints the reference's lines and returns (averages, per-query scores) --
    ``{"map"}, {"ap"}`` under the old protocol ("ok" in gnd[0]), ``{"map_easy", "map_medium", "map_hard"}, {"ap_easy", ...}`` under the
    revisited one (roxford5k* / rparis6k*), None for any other dataset as the reference.  On cuda ranks the three setups are one launch."""
    if "ok" in gnd[0]:
        m, aps, _, _ = compute_map(ranks, gnd)
        print('>> {}: mAP {:.2f}'.format(dataset, np.around(m * 100, decimals=2)))
        return {"map": m}, {"ap": aps}
    if not (dataset.startswith('roxford5k') or dataset.startswith('rparis6k')):
        return None
    setups = _revisited_setups(gnd)
    if torch.is_tensor(ranks) and ranks.is_cuda:
        all_aps, all_prs = average_precision(ranks, setups, kappas)
        per = [(all_aps[s], all_prs[s]) for s in range(3)]
    else:
        per = [_map_host(np.asarray(ranks), g, list(kappas)) for g in setups]
    (mE, mprE), (mM, mprM), (mH, mprH) = [_mean_over_valid(a, p) for a, p in per]
    print('>> {}: mAP E: {}, M: {}, H: {}'.format(dataset, np.around(mE * 100, decimals=2), np.around(mM * 100, decimals=2),
                                                  np.around(mH * 100, decimals=2)))
    print('>> {}: mP@k{} E: {}, M: {}, H: {}'.format(dataset, kappas, np.around(mprE * 100, decimals=2), np.around(mprM * 100, decimals=2),
                                                     np.around(mprH * 100, decimals=2)))
    return {"map_easy": mE, "map_medium": mM, "map_hard": mH}, {"ap_easy": per[0][0], "ap_medium": per[1][0], "ap_hard": per[2][0]}
