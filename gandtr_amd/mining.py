"""An epoch's training tuples, mined on the device -- the inference work the fine-tuning scenario repeats before every epoch
(mdir/examples/iccv23/parameters/finetune.yml: ``CirDiverseAnchors`` for training, ``CirTuples`` for validation, network in ``eval()``
under ``no_grad()``).

Reference: ``TuplesDataset.create_epoch_tuples`` (mdir/external/cirtorch/datasets/traindataset.py:281-303) with the pair selection of
``DiverseAnchorsDataset._select_positive_pairs_db`` (mdir/components/data/dataset/cirtorch_datasets.py:68-115):
    1. descriptors of a query pool                       stages.validate.extract_vectors_from_files
    2. the diverse-anchor selection                      retrieval.select_diverse_anchors
    3. descriptors of the anchors and a negative pool    stages.validate.extract_vectors_from_files
    4. the cluster-aware hard-negative search            retrieval.search_hard_negatives
``name="CirTuples"`` is the plain ``TuplesDataset``: step 1-2 are a random draw of pairs (``select_positive_pairs``, traindataset.py:236-244).
``epoch_tuple_table`` turns the mined index lists into the table of distinct images the tuple loss takes (components/optim/criterion).
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


def _all_or(size, everything):
    """a dataset size of the scenario files: ``.inf`` means all"""
    return everything if size == float("inf") else int(size)


def select_positive_pairs(db, qsize, shuffle, first_neg="neg", nnum=5):
    """``TuplesDataset._select_positive_pairs`` (traindataset.py:236-244): ``qsize`` random pairs of ``db`` (one permutation from torch's
    global generator; the first ``qsize`` pairs without ``shuffle``).  Returns the reference's (qidxs, pidxs, tuple_labels, {})."""
    idxs2qpool = _randperm(len(db["qidxs"]), qsize, shuffle)
    qidxs = [db["qidxs"][i] for i in idxs2qpool]
    pidxs = [db["pidxs"][i] for i in idxs2qpool]
    tuple_labels = ["anc", "pos", first_neg] + ["neg"] * (nnum - 1)
    tuple_labels = [[x] * qsize for x in tuple_labels]
    return qidxs, pidxs, tuple_labels, {}


def epoch_tuple_table(qidxs, pidxs, nidxs, tuple_labels=None):
    """(images, table): the distinct image indices of an epoch's tuples in order of first appearance, and the int32 [T][S] table of
    positions in that list -- column 0 the anchor, 1 the positive, 2.. the negatives (``images[table[t][c]]`` gives the lists back).
    With ``tuple_labels`` ([S][T], as ``create_epoch_tuples`` returns them) the distinct entries are (image index, image label) pairs: an
    image that serves under two labels is listed once per label, because a label-aware network treats the two differently."""
    rows = [[int(q), int(p)] + [int(x) for x in n] for q, p, n in zip(qidxs, pidxs, nidxs)]
    if not rows or any(len(r) != len(rows[0]) for r in rows):
        raise ValueError("an epoch's tuples have one length and there is at least one")
    if tuple_labels is not None:
        rows = [[(i, tuple_labels[c][t]) for c, i in enumerate(r)] for t, r in enumerate(rows)]
    place = {}
    table = [[place.setdefault(i, len(place)) for i in r] for r in rows]
    return list(place), torch.tensor(table, dtype=torch.int32)


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


def create_epoch_tuples(db, images, net, image_size, mean_std, *, qsize, poolsize, nnum, qpool_size=None, similar_exclude=None, similar_include=None,
                        shuffle=True, mark_easy=None, first_neg="neg", clahe_clip=None, extract=None, name="CirDiverseAnchors"):
    """``TuplesDataset.create_epoch_tuples`` for the diverse-anchor dataset (``name="CirDiverseAnchors"``) or the plain one (``"CirTuples"``:
    no ``qpool_size`` / ``similar_*`` / ``mark_easy``; ``qsize`` and ``poolsize`` are capped by what ``db`` and ``images`` hold, as the
    reference's constructor caps them).  A ``qsize`` / ``poolsize`` of ``.inf`` means all pairs / all images.  images: one file (path or contents) per image index; net: the
    embedder on a HIP device; image_size / mean_std / clahe_clip as ``extract_vectors_from_files`` takes them.  ``qpool_size`` None means
    ``qsize``, and it is capped by the number of pairs in ``db`` as the reference's constructor caps it.  ``extract(idxs, label) -> D x N``
    replaces the file path (descriptors that are already known).  Returns (qidxs, pidxs, nidxs, tuple_labels, meta): ``nnum`` negatives per
    tuple from a pool of ``poolsize`` images, meta = {"average_new_query_max_score": [...], "average_negative_distance": [...]}."""
    if extract is None:
        from .stages.validate import extract_vectors_from_files

        def extract(idxs, label):
            with torch.no_grad():
                return extract_vectors_from_files(net, [images[i] for i in idxs], image_size, mean_std, clahe_clip=clahe_clip)
    qsize, poolsize = _all_or(qsize, len(db["qidxs"])), _all_or(poolsize, len(images))
    if name == "CirTuples":
        if qpool_size is not None or similar_exclude is not None or similar_include is not None or mark_easy is not None:
            raise ValueError("CirTuples takes no qpool_size / similar_exclude / similar_include / mark_easy")
        qsize, poolsize = min(qsize, len(db["qidxs"])), min(poolsize, len(images))
        qidxs, pidxs, tuple_labels, pairs_meta = select_positive_pairs(db, qsize, shuffle, first_neg=first_neg, nnum=nnum)
    elif name == "CirDiverseAnchors":
        qpool_size = min(qpool_size, len(db["qidxs"])) if qpool_size is not None else qsize
        qidxs, pidxs, tuple_labels, pairs_meta = select_positive_pairs_diverse(db, qsize, qpool_size, similar_exclude, similar_include, shuffle,
                                                                               extract, mark_easy=mark_easy, first_neg=first_neg, nnum=nnum)
    else:
        raise NotImplementedError("tuple dataset %r is not provided by this build (available: CirDiverseAnchors, CirTuples)" % (name,))
    if nnum == 0:
        return qidxs, pidxs, [[] for _ in range(len(qidxs))], tuple_labels, {**pairs_meta}
    idxs2images = _randperm(len(images), poolsize, shuffle)
    qvecs = extract(qidxs, tuple_labels[0])
    poolvecs = extract(idxs2images, "neg-pool")
    nidxs, neg_meta = retrieval.search_hard_negatives(qidxs, qvecs, idxs2images, poolvecs, db["cluster"], nnum)
    return qidxs, pidxs, nidxs, tuple_labels, {**pairs_meta, **neg_meta}
