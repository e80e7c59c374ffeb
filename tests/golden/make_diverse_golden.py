"""Generate tests/golden/diverse_anchors.npz by calling the reference's own ``DiverseAnchorsDataset._select_positive_pairs_db``
(mdir/components/data/dataset/cirtorch_datasets.py:68-115) unbound on a namespace, the way make_golden.py section 9 calls
``_search_hard_negatives``: the method touches ``qpool_size, similar_exclude, similar_include, mark_easy, shuffle, first_neg, nnum``,
``_randperm`` and ``_extract_descriptors``, so the constructor's pickled database is not needed.  Runs where the reference is (CPU).

A greedy chain turns one flipped pick into a different result, so a case is only usable where the reference's own picks do not hang on
fp32 rounding.  Every case is therefore replayed in float64 and must keep, at every step, a distance of at least GAP = 2e-5 between the
picked similarity and both of its neighbours in the sorted order -- more than twice the worst-case fp32 error of a dot product of unit
vectors, d * 2^-24 = 3.8e-6 at d = 64.  Seeds are screened until a case passes; the assertion runs again on what is written.

Vectors: clustered unit vectors (cluster centres + 0.7 noise, normalised), one per image.  The image at pool position 0 (the first anchor)
has an exact duplicate elsewhere in the pool in the cases marked ``dup``: both sit at the top of the order (similarity 1) from the first
step on, above every target of a case with similar_exclude >= 0.2, so the tie can never decide a pick.

usage:  python tests/golden/make_diverse_golden.py
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden                                                # noqa: E402

GAP = 2e-5

# (d, images, pairs in db, qpool, qsize, exclude, include, shuffle, mark_easy, dup)
CASES = [(32, 400, 300, 300, 40, 0.2, 0.8, False, None, True),
         (16, 330, 260, 200, 60, 0.0, 1.0, True, None, False),       # _randperm shuffles the pool: 200 of 260 pairs
         (32, 200, 120, 120, 120, 0.5, 0.5, False, 0.25, False),     # qsize == qpool, mark_easy
         (64, 400, 300, 257, 64, 0.2, 0.8, True, 0.5, True)]


def make_inputs(seed, d, nimg, npairs, qpool, shuffle, dup):
    rng = np.random.RandomState(seed)
    ncl = max(nimg // 10, 4)
    centres = rng.randn(d, ncl)
    vecs = centres[:, rng.randint(0, ncl, nimg)] + 0.7 * rng.randn(d, nimg)
    perm = rng.permutation(nimg)
    db_q, db_p = perm[:npairs].copy(), rng.permutation(nimg)[:npairs].copy()
    if dup:
        torch.manual_seed(seed)                                       # the pool the reference is going to draw
        pool = torch.randperm(npairs)[:qpool].tolist() if shuffle else list(range(qpool))
        vecs[:, db_q[pool[qpool // 2]]] = vecs[:, db_q[pool[0]]]
    vecs /= np.linalg.norm(vecs, axis=0, keepdims=True)
    return vecs.astype(np.float32), db_q.astype(np.int64), db_p.astype(np.int64)


def min_gap(poolvecs, idxs):
    """float64 replay of the picks ``idxs`` (pool positions): the smallest distance of a picked value to its sorted neighbours"""
    v = poolvecs.astype(np.float64)
    ms = np.full(v.shape[1], -np.inf)
    worst = np.inf
    for t in range(len(idxs) - 1):
        ms = np.maximum(ms, v.T @ v[:, idxs[t]])
        order = np.sort(ms)
        pos = np.searchsorted(order, ms[idxs[t + 1]], side="left")
        assert order[pos] == ms[idxs[t + 1]]
        if pos > 0:
            worst = min(worst, order[pos] - order[pos - 1])
        if pos + 1 < len(order):
            worst = min(worst, order[pos + 1] - order[pos])
    return worst


def run_reference(method, seed, vecs, db_q, db_p, qpool, qsize, exclude, include, shuffle, mark_easy, randperm):
    me = types.SimpleNamespace(qpool_size=qpool, similar_exclude=exclude, similar_include=include, mark_easy=mark_easy, shuffle=shuffle,
                               first_neg="neg", nnum=3)
    me._randperm = lambda size, samples: randperm(me, size, samples)
    me._extract_descriptors = lambda idxs, label, net, device: torch.from_numpy(vecs[:, [int(i) for i in idxs]])
    db = {"qidxs": db_q.tolist(), "pidxs": db_p.tolist()}
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        qidxs, pidxs, labels, meta = method(me, None, None, db, qsize)
    after = int(torch.randint(2 ** 31, (1,)).item())
    return qidxs, pidxs, labels, meta["average_new_query_max_score"], after


def main():
    make_golden._install_placeholders()
    sys.path.insert(0, make_golden.REF)
    threads = torch.get_num_threads()
    import mdir                                                       # noqa: F401
    torch.set_num_threads(threads)
    from mdir.components.data.dataset.cirtorch_datasets import DiverseAnchorsDataset
    from cirtorch.datasets.traindataset import TuplesDataset
    method = DiverseAnchorsDataset._select_positive_pairs_db
    arrays = {"cases": np.array(len(CASES)), "gap": np.array(GAP)}
    for k, (d, nimg, npairs, qpool, qsize, exclude, include, shuffle, mark_easy, dup) in enumerate(CASES):
        for seed in range(1000 * k, 1000 * k + 200):
            vecs, db_q, db_p = make_inputs(seed, d, nimg, npairs, qpool, shuffle, dup)
            qidxs, pidxs, labels, scores, after = run_reference(method, seed, vecs, db_q, db_p, qpool, qsize, exclude, include, shuffle,
                                                                mark_easy, TuplesDataset._randperm)
            # the pool in the reference's order: the images of its anchors are unique, so they give the picked pool positions back
            torch.manual_seed(seed)
            pool = torch.randperm(npairs)[:qpool].tolist() if shuffle else list(range(qpool))
            pool_imgs = [int(db_q[i]) for i in pool]
            idxs = [pool_imgs.index(int(q)) for q in qidxs]
            gap = min_gap(vecs[:, pool_imgs], idxs)
            if gap >= GAP:
                break
        else:
            raise SystemExit("case %d: no seed keeps a gap of %g" % (k, GAP))
        assert min_gap(vecs[:, pool_imgs], idxs) >= GAP
        print("case %d: seed %d, min gap %.3e, %d anchors of %d" % (k, seed, gap, qsize, qpool))
        arrays.update({"c%d_seed" % k: seed, "c%d_vecs" % k: vecs, "c%d_db_qidxs" % k: db_q, "c%d_db_pidxs" % k: db_p,
                       "c%d_qpool" % k: qpool, "c%d_qsize" % k: qsize, "c%d_exclude" % k: exclude, "c%d_include" % k: include,
                       "c%d_shuffle" % k: shuffle, "c%d_mark_easy" % k: np.nan if mark_easy is None else mark_easy, "c%d_dup" % k: dup,
                       "c%d_nnum" % k: 3, "c%d_idxs" % k: np.array(idxs, dtype=np.int64), "c%d_qidxs" % k: np.array(qidxs, dtype=np.int64),
                       "c%d_pidxs" % k: np.array(pidxs, dtype=np.int64), "c%d_labels" % k: np.array(labels),
                       "c%d_scores" % k: np.array(scores, dtype=np.float64), "c%d_randint_after" % k: after, "c%d_min_gap" % k: gap})
    path = os.path.join(HERE, "diverse_anchors.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrays.items()})
    print("wrote diverse_anchors.npz %.1f KiB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
