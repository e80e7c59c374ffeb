"""Generate tests/golden/tuple_loss.npz from the reference's own criteria and pass-through wrapper.  Runs where the reference is (CPU).

Descriptors: per descriptor size d one seeded pool of L2-normalised fp32 vectors in five clusters (unit centres + noise of length 0.35), so
that distances inside a cluster lie around 0.5 -- inside the contrastive margin of 0.75 -- and distances between clusters around 1.4.  A case
is a [T][S] table of pool columns (repeats allowed); the reference receives ``x = pool[:, table.reshape(-1)]`` with the label vector
(-1, 1, 0, ..) per tuple, once tuple by tuple (the way mdir/learning/validation.py:93-107 calls it) and once as a whole batch:
``ContrastiveLoss(0.75)`` and ``TripletLoss(0.1)`` of mdir/components/optim/criterion/cirlosses.py.  Cases: every combination of
d in {8, 100, 2048, 7}, S in {2, 3, 7}, T in {1, 3, 257}, and one crafted table on the d = 100 pool:
    tuple 0   the positive IS the anchor: D = sqrt(d) * eps comes from the eps inside the difference alone;
    tuple 1   every negative beyond the margin (another cluster): zero hinge, the loss is the positive term;
    tuple 2,3 the same anchor vector serves two tuples.
Every stored fp32 result is checked against a float64 evaluation of the same formula on the same fp32 inputs with the bound the tests use
(relative d * 2^-24 on a squared distance, carried through the formula: tests/test_tuple_loss_host.py); a case that missed it would have
to be replaced, not the bound.

Also: 200 image names with the decision of the reference's ``CirRatioPassThrough(0.25, "anc")._passthrough`` for each, and the draws of the
reference's plain ``TuplesDataset._select_positive_pairs`` under a torch seed.

usage:  python tests/golden/make_tuple_loss_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
import make_golden                                                # noqa: E402
from test_tuple_loss_host import float64_losses, bounds           # noqa: E402

POOLS = {8: 300, 100: 300, 2048: 40, 7: 300}
MARGIN_CON, MARGIN_TRI = 0.75, 0.1


def make_pool(d, n, seed):
    rng = np.random.RandomState(seed)
    centres = rng.randn(d, 5)
    centres /= np.linalg.norm(centres, axis=0, keepdims=True)
    cluster = rng.randint(0, 5, n)
    noise = rng.randn(d, n)
    v = centres[:, cluster] + 0.35 * noise / np.linalg.norm(noise, axis=0, keepdims=True)
    v /= np.linalg.norm(v, axis=0, keepdims=True)
    return v.astype(np.float32), cluster


def crafted_table(pool, cluster):
    """four tuples of S = 4 on the d = 100 pool (see the module docstring)"""
    dist = np.linalg.norm(pool[:, :, None].astype(np.float64) - pool[:, None, :].astype(np.float64), axis=0)
    same = lambda i: [j for j in range(pool.shape[1]) if j != i and cluster[j] == cluster[i]]           # noqa: E731
    far = lambda i: [j for j in range(pool.shape[1]) if dist[i, j] > MARGIN_CON + 0.2]                    # noqa: E731
    t0 = [0, 0] + same(0)[:2]
    t1 = [1, same(1)[0]] + far(1)[:2]
    t2 = [2, same(2)[0], same(2)[1], far(2)[0]]
    t3 = [2, same(2)[2], far(2)[1], same(2)[3]]
    return np.array([t0, t1, t2, t3], dtype=np.int32)


def reference_values(crit, x, label, s):
    per_tuple = [float(crit(x[:, i:i + s], label[i:i + s])) for i in range(0, x.shape[1], s)]
    return np.array(per_tuple, dtype=np.float32), np.float32(float(crit(x, label)))


def main():
    make_golden._install_placeholders()
    sys.path.insert(0, make_golden.REF)
    threads = torch.get_num_threads()
    import mdir                                                       # noqa: F401
    torch.set_num_threads(threads)
    from mdir.components.optim.criterion import CRITERIA
    from mdir.components.data.wrapper import CirRatioPassThrough
    from cirtorch.datasets.traindataset import TuplesDataset
    assert "contrastive_multidesc" in CRITERIA and mdir.__file__.startswith(make_golden.REF)      # the reference's package, not this repository's alias
    con, tri = CRITERIA["contrastive"](margin=MARGIN_CON), CRITERIA["triplet"](margin=MARGIN_TRI)
    assert con.reduction == tri.reduction == "sum" and con.eps == 1e-6
    arrays = {"margin_contrastive": np.array(MARGIN_CON), "margin_triplet": np.array(MARGIN_TRI)}
    pools, clusters = {}, {}
    for d, n in POOLS.items():
        pools[d], clusters[d] = make_pool(d, n, 100 + d)
        arrays["pool_d%d" % d] = pools[d]
    cases = [("d%d_s%d_t%d" % (d, s, t), d, None, s, t) for d in POOLS for s in (2, 3, 7) for t in (1, 3, 257)]
    cases.append(("crafted", 100, crafted_table(pools[100], clusters[100]), 4, 4))
    rng = np.random.RandomState(7)
    for name, d, table, s, t in cases:
        if table is None:
            table = rng.randint(0, POOLS[d], (t, s)).astype(np.int32)
        label = torch.tensor(([-1, 1] + [0] * (s - 2)) * t, dtype=torch.float32)
        x = torch.from_numpy(pools[d][:, table.reshape(-1)])
        with torch.no_grad():
            con_tuple, con_batch = reference_values(con, x, label, s)
            tri_tuple, tri_batch = reference_values(tri, x, label, s)
        arrays.update({"%s_table" % name: table, "%s_label" % name: label.numpy(), "%s_con_tuple" % name: con_tuple, "%s_con_batch" % name: con_batch,
                       "%s_tri_tuple" % name: tri_tuple, "%s_tri_batch" % name: tri_batch})
        # the reference's own fp32 results against float64, with the bound of the tests
        for kind, margin, got_tuple, got_batch in ((0, MARGIN_CON, con_tuple, con_batch), (1, MARGIN_TRI, tri_tuple, tri_batch)):
            want = float64_losses(pools[d], table, kind, margin)
            tol = bounds(want, d, kind, margin)
            err = np.abs(got_tuple.astype(np.float64) - want["loss"])
            assert (err <= tol["loss"]).all(), (name, kind, float(err.max()), float(tol["loss"].min()))
            assert abs(float(got_batch) - want["total"]) <= tol["total"], (name, kind)
    arrays["case_names"] = np.array([c[0] for c in cases])
    crafted = arrays["crafted_table"]
    want = float64_losses(pools[100], crafted, 0, MARGIN_CON)
    assert crafted[0, 0] == crafted[0, 1] and abs(want["pair"][0, 0] - 10 * float(np.float32(1e-6))) < 1e-12
    assert (want["pair"][1, 1:] > MARGIN_CON).all() and crafted[2, 0] == crafted[3, 0]
    # the md5 rule of the pass-through wrapper
    names = ["img_%03d" % i for i in range(150)] + ["%032x" % (int(v) * 2654435761 % (1 << 128)) for v in rng.randint(1, 1 << 30, 50)]
    wrapper = CirRatioPassThrough("0.25", "anc", device="cpu")
    arrays["pass_names"] = np.array(names)
    arrays["pass_decisions"] = np.array([bool(wrapper._passthrough(n)) for n in names])
    # the plain pair selection: TuplesDataset._select_positive_pairs unbound on a namespace (the constructor reads a pickle)
    db = {"qidxs": rng.permutation(500)[:120].tolist(), "pidxs": rng.permutation(500)[:120].tolist()}
    for k, (qsize, shuffle) in enumerate(((40, True), (120, True), (25, False))):
        me = types.SimpleNamespace(db=db, qsize=qsize, shuffle=shuffle, first_neg="neg", nnum=5)
        me._randperm = lambda size, samples, me=me: TuplesDataset._randperm(me, size, samples)
        torch.manual_seed(31 + k)
        qidxs, pidxs, labels, meta = TuplesDataset._select_positive_pairs(me, None, None)
        assert meta == {}
        arrays.update({"pairs%d_qsize" % k: qsize, "pairs%d_shuffle" % k: shuffle, "pairs%d_seed" % k: 31 + k,
                       "pairs%d_qidxs" % k: np.array([int(q) for q in qidxs]), "pairs%d_pidxs" % k: np.array([int(p) for p in pidxs]),
                       "pairs%d_labels" % k: np.array(labels), "pairs%d_randint_after" % k: int(torch.randint(2 ** 31, (1,)).item())})
    arrays["pairs_db_qidxs"], arrays["pairs_db_pidxs"], arrays["pairs_cases"] = np.array(db["qidxs"]), np.array(db["pidxs"]), np.array(3)
    path = os.path.join(HERE, "tuple_loss.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrays.items()})
    print("wrote tuple_loss.npz %.1f KiB, %d cases" % (os.path.getsize(path) / 1024, len(cases)))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
