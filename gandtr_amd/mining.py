"""An epoch's training tuples, mined on the device -- the inference work the fine-tuning scenario repeats before every epoch
(mdir/examples/iccv23/parameters/finetune.yml: ``CirDiverseAnchors``, network in ``eval()`` under ``no_grad()``).

Reference: ``TuplesDataset.create_epoch_tuples`` (mdir/external/cirtorch/datasets/traindataset.py:281-303) with the pair selection of
``DiverseAnchorsDataset._select_positive_pairs_db`` (mdir/components/data/dataset/cirtorch_datasets.py:68-115):
    1. descriptors of a query pool                       stages.validate.extract_vectors_from_files
    2. the diverse-anchor selection                      retrieval.select_diverse_anchors
    3. descriptors of the anchors and a negative pool    stages.validate.extract_vectors_from_files
    4. the cluster-aware hard-negative search            retrieval.search_hard_negatives
``db`` is the plain dict the reference unpickles (``qidxs``, ``pidxs``, ``cluster``).  Reading the pickle, ``__getitem__``, the DataLoader
and anything that trains are out of scope.  Random draws come from torch's global generator in the reference's order
(pool permutation, one choice per step, negative-pool permutation): a caller that seeds torch gets the reference's draws.
"""
import torch

from . import retrieval


def _randperm(size, samples, shuffle):
    """``TuplesDataset._randperm`` (traindataset.py:207-210)"""
    if shuffle:
        return torch.randperm(size)[:samples].tolist()
    return list(range(size))[:samples]


def select_positive_pairs_diverse(db, qsize, qpool_size, similar_exclude, similar_include, shuffle, extract, mark_easy=None, first_neg="neg",
                                  nnum=5, mine_label="pool"):
    """``DiverseAnchorsDataset._select_positive_pairs_db``.  ``extract(idxs, label) -> D x N`` gives the descriptors of the images ``idxs``
    (label: the reference's image label, "anc-pool" / "pos-pool").  A pool of ``qpool_size`` pairs is drawn, ``qsize`` diverse anchors are
    picked from it (``retrieval.select_diverse_anchors``), and with ``mark_easy`` the pairs are labelled by their anchor-positive
    similarity: the ``int(mark_easy * qsize)`` most similar "-easy", the rest "-hard" (a count of zero marks all of them easy: the
    reference's ``sim_ord[-0:]``).  Returns the reference's (qidxs, pidxs, tuple_labels, {"average_new_query_max_score": [...]})."""
    assert similar_exclude <= similar_include
    assert mark_easy is None or 0 <= mark_easy <= 1
    assert qsize <= qpool_size
    if qpool_size > len(db["qidxs"]):
        raise ValueError("a query pool of %d from %d pairs" % (qpool_size, len(db["qidxs"])))
    idxs2qpool = _randperm(len(db["qidxs"]), qpool_size, shuffle)
    qidxs = [db["qidxs"][i] for i in idxs2qpool]
    pidxs = [db["pidxs"][i] for i in idxs2qpool]
    qvecs = extract(qidxs, "anc-%s" % mine_label)
    idxs, qscore_acc = retrieval.select_diverse_anchors(qvecs, qsize, similar_exclude, similar_include, shuffle)
    qidxs = [qidxs[x] for x in idxs]
    pidxs = [pidxs[x] for x in idxs]
    difficulties = [""] * len(qidxs)
    if mark_easy is not None:
        with torch.no_grad():
            qvecs = qvecs[:, idxs]
            pvecs = extract(pidxs, "pos-%s" % mine_label)
            sim_ord = (qvecs * pvecs).sum(0).argsort()
        easy_set = set(sim_ord[-int(mark_easy * qsize):].tolist())
        difficulties = ["-easy" if i in easy_set else "-hard" for i in range(len(qidxs))]
    tuple_labels = ["anc", "pos", first_neg] + ["neg"] * (nnum - 1)
    tuple_labels = [[x + y for y in difficulties] for x in tuple_labels]
    return qidxs, pidxs, tuple_labels, {"average_new_query_max_score": qscore_acc}


def create_epoch_tuples(db, images, net, image_size, mean_std, *, qsize, poolsize, nnum, qpool_size, similar_exclude, similar_include,
                        shuffle=True, mark_easy=None, first_neg="neg", clahe_clip=None, extract=None):
    """``TuplesDataset.create_epoch_tuples`` for the diverse-anchor dataset.  images: one file (path or contents) per image index; net: the
    embedder on a HIP device; image_size / mean_std / clahe_clip as ``extract_vectors_from_files`` takes them.  ``qpool_size`` None means
    ``qsize``, and it is capped by the number of pairs in ``db`` as the reference's constructor caps it.  ``extract(idxs, label) -> D x N``
    replaces the file path (descriptors that are already known).  Returns (qidxs, pidxs, nidxs, tuple_labels, meta): ``nnum`` negatives per
    tuple from a pool of ``poolsize`` images, meta = {"average_new_query_max_score": [...], "average_negative_distance": [...]}."""
    if extract is None:
        from .stages.validate import extract_vectors_from_files

        def extract(idxs, label):
            with torch.no_grad():
                return extract_vectors_from_files(net, [images[i] for i in idxs], image_size, mean_std, clahe_clip=clahe_clip)
    qpool_size = min(qpool_size, len(db["qidxs"])) if qpool_size is not None else qsize
    qidxs, pidxs, tuple_labels, pairs_meta = select_positive_pairs_diverse(db, qsize, qpool_size, similar_exclude, similar_include, shuffle,
                                                                           extract, mark_easy=mark_easy, first_neg=first_neg, nnum=nnum)
    if nnum == 0:
        return qidxs, pidxs, [[] for _ in range(len(qidxs))], tuple_labels, {**pairs_meta}
    idxs2images = _randperm(len(images), poolsize, shuffle)
    qvecs = extract(qidxs, tuple_labels[0])
    poolvecs = extract(idxs2images, "neg-pool")
    nidxs, neg_meta = retrieval.search_hard_negatives(qidxs, qvecs, idxs2images, poolvecs, db["cluster"], nnum)
    return qidxs, pidxs, nidxs, tuple_labels, {**pairs_meta, **neg_meta}
