"""Functions of the grouping layers (interface of mdir/components/model/layers/functional.py): L2 normalisation, the soft-assignment weights,
Forgy initialisation and the clustering iterations.  On CPU tensors everything is the reference's formula in torch ops; ``iterate_kmeans`` on
HIP tensors runs on the device (gandtr_amd/codebook.py).

Deviation (k-means): a cluster that loses all its points KEEPS its centroid.  In the reference ``torch.mean`` of the empty selection is NaN,
``torch.min`` then returns the NaN's index for every point and one iteration later the whole codebook is NaN."""
import torch


def normalize_vec_l2(vec):
    """v / (||v|| + 1e-6) along the last dimension"""
    return vec / (torch.norm(vec, dim=-1, keepdim=True) + 1e-6)


def idx2rank_dim1(idxs):
    """Indices along dim 1 (an argsort) -> the rank of every column"""
    ranks = torch.zeros_like(idxs)
    order = torch.arange(idxs.shape[1], device=idxs.device)
    for row, idx in zip(ranks, idxs):
        row[idx] = order
    return ranks


def assign_weights_softmax(dists, base):
    """softmax(-base * distance) over the centroids (dim 1)"""
    return torch.nn.functional.softmax(-base * dists, dim=1)


def assign_weights_cmeans(dists, fuzzifier, eps):
    """Fuzzy c-means membership: 1 / sum_k ((d_j + e) / (d_k + e)) ** (2 / (m - 1)) with e = eps ** ((m - 1) / 2)"""
    shifted = dists.unsqueeze(2).repeat_interleave(dists.shape[1], dim=2) + eps ** ((fuzzifier - 1) / 2)
    return 1 / shifted.div(shifted.transpose(1, 2)).pow(2 / (fuzzifier - 1)).sum(-1)


def init_clusters_forgy(points, n_clusters):
    """Forgy initialisation: n_clusters of the points, drawn by a host-side ``torch.randperm`` (the same ``torch.manual_seed`` picks the same
    points whatever device they live on)"""
    return points[torch.randperm(points.shape[0])[:n_clusters].to(points.device)]


def iterate_kmeans(points, clusters, iterations):
    """Lloyd iterations, updating ``clusters`` in place where its layout allows.  HIP tensors: iterations x (gdt_codebook_nearest,
    gdt_kmeans_update), inference only.  A cluster without points keeps its centroid (module docstring)."""
    if points.is_cuda:
        from .... import codebook
        work = clusters.detach()
        if not (work.dtype == torch.float32 and work.is_contiguous()):
            work = work.float().contiguous()
        for _ in range(iterations):
            _, ids = codebook.nearest(points, work, 1)
            codebook.kmeans_update(points, ids, work)
        if work.data_ptr() != clusters.data_ptr():
            clusters = work
        return clusters
    for _ in range(iterations):
        _, assignment = torch.min(torch.cdist(points, clusters), dim=1)
        for ctr in range(clusters.shape[0]):
            members = points[assignment == ctr]
            if members.shape[0]:
                clusters[ctr] = torch.mean(members, dim=0)
    return clusters


def iterate_cmeans(points, clusters, iterations, fuzzifier, eps):
    """Fuzzy c-means iterations"""
    for _ in range(iterations):
        weights = torch.pow(assign_weights_cmeans(torch.cdist(points, clusters), fuzzifier, eps), fuzzifier).T
        clusters = weights.mm(points) / (weights.sum(-1, keepdim=True) + eps)
    return clusters


def iterate_softmax(points, clusters, iterations, base, eps):
    """Soft k-means iterations with softmax weights raised to ``base``"""
    for _ in range(iterations):
        weights = torch.pow(assign_weights_softmax(torch.cdist(points, clusters), base), base).T
        clusters = weights.mm(points) / (weights.sum(-1, keepdim=True) + eps)
    return clusters


def cluster_faiss(points, n_clusters):
    """The reference clusters with faiss through the ``asmk`` package, which this repository does not ship"""
    raise ImportError("asmk (faiss clustering) is not available; use ClusteringCodebook (Forgy initialisation + iterate_kmeans)")
