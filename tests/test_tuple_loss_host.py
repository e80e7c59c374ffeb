"""The loss validation of the fine-tuning scenario on the host (no GPU): the torch branch of the criteria against what the reference's own
criteria returned (tests/golden/tuple_loss.npz, written by tests/golden/make_tuple_loss_golden.py), the pass-through wrappers, the plain
pair selection, the tuple table, the construction of finetune.yml's ``network.augment`` wrappers and ``learning.validation`` section, and
the C entry's argument checks.

Tolerance (``bounds``), derived and not fitted.  The inputs are fp32 and the float64 evaluation (``float64_losses``) of the same formula
on the same fp32 inputs (eps = fp32(1e-6), what an fp32 computation adds) is taken as exact.  The only fp32 error source that grows with
the problem is the sum over the d elements of a row: the squared distance q carries a relative error of at most r = d * 2^-24.  Carried
through the formulas:
    contrastive   D = sqrt(q):            |dD| <= D (1 - sqrt(1 - r))                                  (about D r / 2)
                  positive  0.5 D^2 = q/2: |d|  <= r q / 2
                  negative  0.5 h^2, h = max(margin - D, 0), decreasing in D:  |d| <= 0.5 (max(margin - D + dD, 0)^2 - h^2)
    triplet       max(q_ap - q_an + margin, 0) is 1-Lipschitz in both:          |d| <= r (q_ap + q_an)
    a tuple's loss: the sum of its terms' bounds;  the total: the sum of the tuples' bounds.
``test_reference_fp32_sits_inside_the_bound`` confirms that the reference's own fp32 torch results obey it on every fixture case."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gandtr_amd import mining, retrieval
from gandtr_amd.components.data import wrapper as W
from gandtr_amd.components.optim import criterion as C
from gandtr_amd.tools import tensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tuple_loss.npz")
EPS = float(np.float32(1e-6))

# mdir/examples/iccv23/parameters/finetune.yml: network.augment.runtime.wrappers, learning.validation, data.val, learning.training.criterion
FINETUNE_WRAPPERS = ("meanstd_post:[[0.5,0.5,0.5],[0.5,0.5,0.5]]:[[0.485,0.456,0.406],[0.229,0.224,0.225]],"
                     "clahepost:[[0.5,0.5,0.5],[0.5,0.5,0.5]]:1.0,cir_ratio_pass_through:0.25:anc")
FINETUNE_VALIDATION = {"criterion": "default", "data": "val", "frequency": 5, "network_overlay": None, "type": "SingleValidation"}
FINETUNE_DATA_VAL = {"dataset": {"dataset": "retrieval-SfM-120k", "dataset_pkl": None, "image_dir": "data/train/retrieval-SfM-120k/ims/*",
                                 "image_size": 362, "name": "CirTuples", "neg_num": 5, "pool_size": float("inf"), "query_size": float("inf"),
                                 "split": "val"},
                     "loader": {"batch_size": 1}}
FINETUNE_CRITERION = {"loss": "contrastive", "margin": 0.75}
FINETUNE_EMBED_DATA = {"transforms": "pil2np | apply_clahe:1.0 | totensor | normalize", "mean_std": [[0.485, 0.456, 0.406], [0.229, 0.224, 0.225]]}


def float64_losses(pool, table, kind, margin):
    """the formulas of functional.py:141-173 in float64 on fp32 inputs.  pool: [d][n] fp32, table: [T][S] columns of pool.
    -> {"sq": squared distances [T][S-1], "pair": what gdt_tuple_loss calls pair_dist, "loss": [T], "total"}"""
    v = np.asarray(pool, dtype=np.float64).T
    table = np.asarray(table)
    dif = v[table[:, :1]] - v[table[:, 1:]]
    if kind == 0:
        sq = ((dif + EPS) ** 2).sum(-1)
        pair = np.sqrt(sq)
        terms = 0.5 * np.maximum(margin - pair, 0) ** 2
        terms[:, 0] = 0.5 * pair[:, 0] ** 2
    else:
        sq = (dif ** 2).sum(-1)
        pair = sq
        terms = np.maximum(sq[:, :1] - sq[:, 1:] + margin, 0)
    loss = terms.sum(-1)
    return {"sq": sq, "pair": pair, "loss": loss, "total": float(loss.sum())}


def bounds(want, d, kind, margin):
    """the module docstring's bound for every output: {"pair": [T][S-1], "loss": [T], "total"}"""
    r = d * 2.0 ** -24
    sq = want["sq"]
    if kind == 0:
        dist = want["pair"]
        d_dist = dist * (1 - np.sqrt(1 - r))
        h = np.maximum(margin - dist, 0)
        terms = 0.5 * (np.maximum(margin - dist + d_dist, 0) ** 2 - h ** 2)
        terms[:, 0] = 0.5 * r * sq[:, 0]
        pair = d_dist
    else:
        pair = r * sq
        terms = r * (sq[:, :1] + sq[:, 1:])
    loss = terms.sum(-1)
    return {"pair": pair, "loss": loss, "total": float(loss.sum())}


def load_cases():
    g = np.load(GOLDEN)
    cases = []
    for name in [str(n) for n in g["case_names"]]:
        table = g[name + "_table"]
        d = 100 if name == "crafted" else int(name.split("_")[0][1:])
        cases.append({"name": name, "d": d, "pool": g["pool_d%d" % d], "table": table, "label": g[name + "_label"],
                      0: (float(g["margin_contrastive"]), g[name + "_con_tuple"], float(g[name + "_con_batch"])),
                      1: (float(g["margin_triplet"]), g[name + "_tri_tuple"], float(g[name + "_tri_batch"]))})
    return cases


def criterion_of(kind, margin):
    return C.ContrastiveLoss(margin) if kind == 0 else C.TripletLoss(margin)


def test_fixture_covers_what_it_must():
    cases = {c["name"]: c for c in load_cases()}
    for d in (8, 100, 2048, 7):
        for s in (2, 3, 7):
            for t in (1, 3, 257):
                assert cases["d%d_s%d_t%d" % (d, s, t)]["table"].shape == (t, s)
    for c in cases.values():
        norms = np.linalg.norm(c["pool"].astype(np.float64), axis=0)
        assert c["pool"].dtype == np.float32 and np.abs(norms - 1).max() < 1e-6
        assert c["label"].tolist() == ([-1, 1] + [0] * (c["table"].shape[1] - 2)) * c["table"].shape[0]
    crafted = cases["crafted"]
    table, want = crafted["table"], float64_losses(crafted["pool"], crafted["table"], 0, 0.75)
    assert table[0, 0] == table[0, 1]                                     # the positive is the anchor: eps alone decides D = sqrt(d) eps
    assert want["pair"][0, 0] == pytest.approx(10 * EPS, rel=1e-12) and want["pair"][0, 0] > 0
    assert (want["pair"][1, 1:] > 0.75).all()                             # zero hinge: the loss is the positive term alone
    assert want["loss"][1] == pytest.approx(0.5 * want["sq"][1, 0], rel=1e-14)
    assert table[2, 0] == table[3, 0] and table[2].tolist() != table[3].tolist()      # one vector serves two tuples
    active = sum(int(((float64_losses(c["pool"], c["table"], 0, 0.75)["pair"][:, 1:]) < 0.75).sum()) for c in cases.values())
    assert active > 100                                                   # negatives inside the margin exist: the hinge is exercised
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("kind", [0, 1])
def test_reference_fp32_sits_inside_the_bound(kind):
    """the reference's own fp32 torch results against float64: the bound is one the reference itself keeps"""
    worst = 0.0
    for c in load_cases():
        margin, ref_tuple, ref_batch = c[kind]
        want = float64_losses(c["pool"], c["table"], kind, margin)
        tol = bounds(want, c["d"], kind, margin)
        err = np.abs(ref_tuple.astype(np.float64) - want["loss"])
        assert (err <= tol["loss"]).all(), c["name"]
        assert abs(ref_batch - want["total"]) <= tol["total"], c["name"]
        worst = max(worst, float((err / np.maximum(tol["loss"], 1e-300)).max()))
    print("kind %d: the reference uses at most %.3f of the bound" % (kind, worst))


@pytest.mark.parametrize("kind", [0, 1])
def test_torch_branch_reproduces_the_reference(kind):
    for c in load_cases():
        margin, ref_tuple, ref_batch = c[kind]
        crit = criterion_of(kind, margin)
        want = float64_losses(c["pool"], c["table"], kind, margin)
        tol = bounds(want, c["d"], kind, margin)
        pool = torch.from_numpy(c["pool"])
        got = crit.tuple_losses(pool, c["table"], with_pairs=True)
        assert got.loss.dtype == torch.float32 and got.total.dtype == torch.float64
        assert (np.abs(got.loss.double().numpy() - want["loss"]) <= tol["loss"]).all(), c["name"]
        assert (np.abs(got.pair_dist.double().numpy() - want["pair"]) <= tol["pair"]).all(), c["name"]
        assert abs(float(got.total) - want["total"]) <= tol["total"]
        # both fp32 results lie within the bound of float64, hence within twice the bound of each other
        assert (np.abs(got.loss.double().numpy() - ref_tuple) <= 2 * tol["loss"]).all(), c["name"]
        # the label form on the gathered columns, as the reference is called; a list of label tensors is concatenated (cirlosses.py:17-20)
        x = pool[:, torch.from_numpy(c["table"].reshape(-1)).long()]
        label = torch.from_numpy(c["label"])
        batch = crit(x, label)
        assert batch.dim() == 0 and batch.dtype == torch.float32
        assert abs(float(batch) - want["total"]) <= tol["total"] + abs(want["total"]) * 2.0 ** -24       # + the final rounding to fp32
        assert abs(float(batch) - ref_batch) <= 2 * tol["total"] + abs(want["total"]) * 2.0 ** -23
        s = c["table"].shape[1]
        assert float(crit(x, [label[i:i + s] for i in range(0, len(label), s)])) == float(batch)


def test_criterion_registry_and_errors():
    assert set(C.CRITERIA) == {"contrastive", "triplet"}
    con = C.initialize_criterion(dict(FINETUNE_CRITERION))
    assert isinstance(con, C.ContrastiveLoss) and con.margin == 0.75 and con.eps == 1e-6 and con.reduction == "sum"
    assert repr(con) == "ContrastiveLoss(margin=0.7500)"
    tri = C.initialize_criterion({"loss": "triplet", "margin": 0.1})
    assert isinstance(tri, C.TripletLoss) and tri.reduction == "sum" and repr(tri) == "TripletLoss(margin=0.1000)"
    assert C.initialize_criterion({}) is None and C.initialize_criterion(None) is None
    with pytest.raises(NotImplementedError):
        C.initialize_criterion({"loss": "contrastive_multidesc", "margin": 0.7, "weights": None})
    with pytest.warns(DeprecationWarning):
        assert C.ContrastiveLoss(0.7, eps=1e-3).eps == 1e-6
    x = torch.nn.functional.normalize(torch.randn(8, 6, generator=torch.Generator().manual_seed(0)), dim=0)
    for bad in ([[0, 6]], [[-1, 2]], [[0]], [], [[0.5, 1.0]]):
        with pytest.raises(ValueError):
            con.tuple_losses(x, bad)
    for bad in ([-1, 1, 0, -1, 0, 1], [1, -1, 0, 1, -1, 0], [-1, 1, 0, 0], [0] * 6, [-1, 1, 0, -1, 1, 1]):
        with pytest.raises(ValueError):
            con(x, torch.tensor(bad, dtype=torch.float32))
    with pytest.raises(ValueError):                                    # the device entry takes device descriptors only: no silent host run
        C.tuple_loss_hip(x, [[0, 1]], 0, 0.75, 1e-6)
    assert float(tri(x[:, :4], torch.tensor([-1., 1, -1, 1]))) == 0.0      # S == 2: a triplet loss without negatives has no terms


def test_pass_through_decisions_equal_the_references():
    g = np.load(GOLDEN)
    names, decisions = [str(n) for n in g["pass_names"]], g["pass_decisions"].tolist()
    assert len(names) == 200 and 20 < sum(decisions) < 80
    wrap = W.CirRatioPassThrough("0.25", "anc", device="cpu")
    assert [wrap._passthrough(n) for n in names] == decisions
    assert wrap._passthrough([names[0]]) == decisions[0]               # a collated batch of one
    assert repr(wrap) == "CirRatioPassThrough(probability=0.25, train_label=%r)" % re.compile("anc")


def test_finetune_wrapper_string_builds():
    """finetune.yml's network.augment.runtime.wrappers (a KeyError before the two pass-through wrappers existed)"""
    chain = W.initialize_wrappers(FINETUNE_WRAPPERS, "cpu")
    assert [type(w).__name__ for w in chain.wrappers] == ["MeanStdPost", "ClahePost", "CirRatioPassThrough"]
    assert chain.wrappers[2].probability == 0.25 and chain.wrappers[2].image_label.pattern == "anc"
    assert W.WRAPPERS_LABELS["random_pass_through"] is W.RandomPassThrough
    assert isinstance(W.initialize_wrappers("random_pass_through:0.5", "cpu").wrappers[0], W.RandomPassThrough)


def _labelled(i, label, shape=(1, 3, 4, 4)):
    return tensors.as_metadata_tensor(torch.full(shape, float(i)), {"image_label": label, "name": "img_%03d" % i})


def test_cir_ratio_pass_through_single_list_and_batch():
    g = np.load(GOLDEN)
    decision = dict(zip([str(n) for n in g["pass_names"]], g["pass_decisions"].tolist()))
    wrap = W.CirRatioPassThrough("0.25", "anc", device="cpu")
    net = lambda x: x + 100                                            # noqa: E731
    # one image: the reference's two outcomes; "anc-mine" matches (re.match), "pos" and "neg-pool-mine" do not
    for i in range(12):
        for label in ("anc", "anc-mine", "pos", "neg-pool-mine"):
            x = _labelled(i, label)
            pre, meta = wrap.preprocess(x, None)
            through = label.startswith("anc") and decision["img_%03d" % i]
            assert (pre is not None) == through
            out = wrap.postprocess(None if pre is None else net(tensors.as_tensor(pre)), None, meta)
            assert torch.equal(out, x.tensor + (100 if through else 0))
    # a list: the per-item loop's result, the passing items batched by size (two sizes, at most max_batch rows per batch)
    items = [_labelled(i, "anc" if i % 3 else "pos", (1, 3, 4, 4 + 2 * (i % 2))) for i in range(150)]
    want = [x.tensor + (100 if (i % 3 and decision["img_%03d" % i]) else 0) for i, x in enumerate(items)]
    pre, meta = wrap.preprocess(items, None)
    passing = sum(1 for i in range(150) if i % 3 and decision["img_%03d" % i])
    assert sum(p.shape[0] for p in pre) == passing and all(p.shape[0] <= wrap.max_batch for p in pre)
    assert len(pre) < passing and len({tuple(p.shape[1:]) for p in pre}) == 2
    out = wrap.postprocess([net(p) for p in pre], None, meta)
    assert len(out) == 150 and all(torch.equal(a, b) for a, b in zip(out, want))
    # nobody passes: an empty list goes to the network, everything is put back
    pre, meta = wrap.preprocess(items[::3], None)
    assert pre == [] and all(torch.equal(a, b.tensor) for a, b in zip(wrap.postprocess([], None, meta), items[::3]))
    # a batch with one metadata entry per row: decided row by row, written back over a copy of the input
    rows = list(range(20))
    batch = tensors.MetadataTensor(torch.cat([items[i].tensor[:, :, :, :4] for i in rows]),
                                   {"image_label": [items[i].metadata["image_label"] for i in rows], "name": ["img_%03d" % i for i in rows]})
    before = batch.tensor.clone()
    pre, meta = wrap.preprocess(batch, None)
    take = [i for i in rows if i % 3 and decision["img_%03d" % i]]
    assert 0 < len(take) < 20 and pre.shape[0] == len(take)
    out = wrap.postprocess(net(pre), None, meta)
    assert torch.equal(out, torch.cat([want[i][:, :, :, :4] for i in rows])) and torch.equal(batch.tensor, before)


def test_random_pass_through_draws_in_input_order():
    import random
    wrap = W.RandomPassThrough("0.4", device="cpu")
    items = [torch.full((1, 3, 2, 2), float(i)) for i in range(30)]
    random.seed(4)
    pre, meta = wrap.preprocess(items, None)
    out = wrap.postprocess([p + 100 for p in pre], None, meta)
    random.seed(4)
    want = [x + 100 if random.random() < 0.4 else x for x in items]
    assert all(torch.equal(a, b) for a, b in zip(out, want))


def test_epoch_tuple_table_round_trips():
    qidxs, pidxs, nidxs = [5, 6, 5], [7, 5, 8], [[1, 2], [2, 9], [7, 1]]
    images, table = mining.epoch_tuple_table(qidxs, pidxs, nidxs)
    assert images == [5, 7, 1, 2, 6, 9, 8] and table.dtype == torch.int32 and table.shape == (3, 4)
    back = [[images[i] for i in row] for row in table.tolist()]
    assert back == [[q, p] + n for q, p, n in zip(qidxs, pidxs, nidxs)]
    # with image labels an image under two labels is listed once per label
    labels = [["anc"] * 3, ["pos"] * 3, ["neg"] * 3, ["neg"] * 3]
    entries, table = mining.epoch_tuple_table(qidxs, pidxs, nidxs, labels)
    assert len(entries) == len(set(entries)) == 9 and (5, "anc") in entries and (5, "pos") in entries and (7, "pos") in entries and (7, "neg") in entries
    assert [[entries[i] for i in row] for row in table.tolist()] == [[(q, "anc"), (p, "pos")] + [(x, "neg") for x in n]
                                                                      for q, p, n in zip(qidxs, pidxs, nidxs)]
    assert table[0, 0] == table[2, 0]                                      # the anchor of tuples 0 and 2 is embedded once
    with pytest.raises(ValueError):
        mining.epoch_tuple_table([], [], [])
    with pytest.raises(ValueError):
        mining.epoch_tuple_table([1, 2], [3, 4], [[5], [6, 7]])


def test_plain_pair_selection_reproduces_the_references_draws():
    g = np.load(GOLDEN)
    db = {"qidxs": g["pairs_db_qidxs"].tolist(), "pidxs": g["pairs_db_pidxs"].tolist()}
    for k in range(int(g["pairs_cases"])):
        qsize, shuffle = int(g["pairs%d_qsize" % k]), bool(g["pairs%d_shuffle" % k])
        torch.manual_seed(int(g["pairs%d_seed" % k]))
        qidxs, pidxs, labels, meta = mining.select_positive_pairs(db, qsize, shuffle, first_neg="neg", nnum=5)
        assert qidxs == g["pairs%d_qidxs" % k].tolist() and pidxs == g["pairs%d_pidxs" % k].tolist()
        assert labels == g["pairs%d_labels" % k].tolist() and meta == {}
        assert int(torch.randint(2 ** 31, (1,)).item()) == int(g["pairs%d_randint_after" % k])


def _host_hard_negatives(qidxs, qvecs, idxs2images, poolvecs, clusters, nnum):
    """traindataset.py:246-279 on the host (oracle/retrieval_oracle.py)"""
    from oracle import retrieval_oracle as R
    nidxs, dist = R.search_hard_negatives(list(qidxs), qvecs.numpy(), list(idxs2images), poolvecs.numpy(), list(clusters), nnum)
    return [list(map(int, n)) for n in nidxs], {"average_negative_distance": [float(x) for x in np.asarray(dist).reshape(-1)]}


def test_create_epoch_tuples_serves_cir_tuples(monkeypatch):
    monkeypatch.setattr(retrieval, "search_hard_negatives", _host_hard_negatives)
    rng = np.random.RandomState(3)
    nimg, npairs = 90, 40
    vecs = torch.nn.functional.normalize(torch.from_numpy(rng.randn(16, nimg).astype(np.float32)), dim=0)
    db = {"qidxs": rng.permutation(nimg)[:npairs].tolist(), "pidxs": rng.permutation(nimg)[:npairs].tolist(), "cluster": rng.randint(0, 20, nimg).tolist()}
    calls = []

    def extract(idxs, label):
        calls.append((len(idxs), label if isinstance(label, str) else list(label)))
        return vecs[:, idxs]
    torch.manual_seed(2)
    qidxs, pidxs, nidxs, labels, meta = mining.create_epoch_tuples(db, [None] * nimg, None, 64, None, extract=extract, name="CirTuples",
                                                                   qsize=float("inf"), poolsize=float("inf"), nnum=3)
    torch.manual_seed(2)
    pool = torch.randperm(npairs).tolist()                                # .inf: all pairs, all images
    assert qidxs == [db["qidxs"][i] for i in pool] and pidxs == [db["pidxs"][i] for i in pool]
    images = torch.randperm(nimg).tolist()
    want_n, want_meta = _host_hard_negatives(qidxs, vecs[:, qidxs], images, vecs[:, images], db["cluster"], 3)
    assert nidxs == want_n and meta == want_meta
    assert labels == [["anc"] * npairs, ["pos"] * npairs, ["neg"] * npairs, ["neg"] * npairs, ["neg"] * npairs]
    assert calls == [(npairs, ["anc"] * npairs), (nimg, "neg-pool")]
    qidxs, _, _, _, _ = mining.create_epoch_tuples(db, [None] * nimg, None, 64, None, extract=extract, name="CirTuples", qsize=1000, poolsize=50,
                                                   nnum=2, shuffle=False)
    assert qidxs == db["qidxs"]                                          # capped by the pairs there are, as the reference's constructor does
    with pytest.raises(ValueError):
        mining.create_epoch_tuples(db, [None] * nimg, None, 64, None, extract=extract, name="CirTuples", qsize=5, poolsize=50, nnum=2, qpool_size=9)
    with pytest.raises(NotImplementedError):
        mining.create_epoch_tuples(db, [None] * nimg, None, 64, None, extract=extract, name="CirOther", qsize=5, poolsize=50, nnum=2)


class _MeanNet:
    """a stand-in network on the CPU: the descriptor of an image is a fixed projection of its pixels, shifted for the images whose label and
    name pass ``CirRatioPassThrough(0.25, "anc")`` -- it records the metadata it is handed"""

    class _Params:
        runtime = {"data": dict(FINETUNE_EMBED_DATA)}
    network_params = _Params
    meta = {"out_channels": 8}
    device = torch.device("cpu")

    def __init__(self):
        self.rule = W.CirRatioPassThrough("0.25", "anc", device="cpu")
        self.seen = []
        self.proj = torch.randn(8, 3 * 8 * 8, generator=torch.Generator().manual_seed(1))

    def eval(self):
        return self

    def overlay_params(self, params, device):
        return self

    def __call__(self, x):
        label, name = x.metadata["image_label"], x.metadata["name"]
        self.seen.append((label[0], name[0]))
        v = self.proj @ x.tensor.reshape(-1)
        if self.rule._decision(label[0], name[0]):
            v = v.flip(0)
        return torch.nn.functional.normalize(v, dim=0)


def test_finetune_validation_section_builds_and_runs_on_the_host(monkeypatch):
    """finetune.yml's learning.validation (a NotImplementedError before): built from the file's own keys, run with a stand-in network"""
    from gandtr_amd.learning.validation import SingleValidation, TuplesData, initialize_validation
    monkeypatch.setattr(retrieval, "search_hard_negatives", _host_hard_negatives)
    nimg = 24
    gen = torch.Generator().manual_seed(5)
    images = [torch.randn(3, 8, 8, generator=gen) for _ in range(nimg)]
    db = {"qidxs": list(range(0, 10)), "pidxs": [i + 10 for i in range(10)], "cluster": [i % 10 for i in range(nimg)],
          "cids": ["img_%03d" % i for i in range(nimg)]}
    net, default = _MeanNet(), C.initialize_criterion(dict(FINETUNE_CRITERION))
    val = initialize_validation(copy.deepcopy(FINETUNE_VALIDATION), data={"db": db, "images": images}, params_data={"val": copy.deepcopy(FINETUNE_DATA_VAL)},
                                default_criterion=default, network=net)
    assert isinstance(val, SingleValidation) and isinstance(val.data_loader, TuplesData) and val.criterion is default
    assert val.decisive_criterion == "val/learning/loss:total" and val.criterion_mean_reduction is False and val.frequency == 5
    assert len(val.data_loader) == 10 and val.validations(4) == [("val", val)] and val.validations(0) == []
    assert "CirTuples" in repr(val) and "ContrastiveLoss(margin=0.7500)" in repr(val)
    rows = []
    torch.manual_seed(0)
    acc = val.validate(net, torch.device("cpu"), lambda *row: rows.append(row))
    assert isinstance(acc, list) and len(acc) == 10 and all(isinstance(x, float) and np.isfinite(x) for x in acc)
    data = val.data_loader
    assert sorted(data.qidxs) == db["qidxs"] and all(len(n) == 5 for n in data.nidxs)
    # the labels that reached the network: "-mine" while mining (anchors, then the negative pool), the tuple labels afterwards, once per (image, label)
    mined = net.seen[:10 + nimg]
    assert mined[:10] == [("anc-mine", "img_%03d" % q) for q in data.qidxs] and {l for l, _ in mined[10:]} == {"neg-pool-mine"}
    entries, table = mining.epoch_tuple_table(data.qidxs, data.pidxs, data.nidxs, data.tuple_labels)
    assert net.seen[10 + nimg:] == [(label, "img_%03d" % i) for i, label in entries] and len(set(entries)) == len(entries)
    # the losses: the criterion on the descriptors of the tuples' images, tuple by tuple as the reference's loop scores them
    for t, loss in enumerate(acc):
        cols = [net(tensors.MetadataTensor(images[i][None], {"image_label": [l], "name": ["img_%03d" % i]})) for i, l in (entries[k] for k in table[t].tolist())]
        one = float(default(torch.stack(cols, 1), torch.tensor([-1., 1, 0, 0, 0, 0, 0])))
        assert loss == pytest.approx(one, rel=1e-5, abs=1e-9)
    # what is logged: the mining metadata once, one loss row per tuple
    kinds = [(r[2], r[4]) for r in rows]
    assert kinds[0] == ("data_mining", "scalar/loss") and set(rows[0][3]) == {"average_negative_distance"} and rows[0][0] is None
    assert [r[3]["total"] for r in rows if r[2] == "loss"] == acc and [r[0] for r in rows if r[2] == "loss"] == list(range(10))
    # a criterion section of its own goes through initialize_criterion; data: null still builds a score; unknown datasets are refused
    own = dict(copy.deepcopy(FINETUNE_VALIDATION), criterion={"loss": "triplet", "margin": 0.1})
    val2 = initialize_validation(own, data={"db": db, "images": images}, params_data={"val": copy.deepcopy(FINETUNE_DATA_VAL)}, default_criterion=None,
                                 network=net)
    assert isinstance(val2.criterion, C.TripletLoss) and val2.decisive_criterion == "val/learning/loss:total"
    with pytest.raises(ValueError):
        initialize_validation(copy.deepcopy(FINETUNE_VALIDATION), data={"db": db, "images": images}, params_data={"val": copy.deepcopy(FINETUNE_DATA_VAL)},
                              default_criterion=None, network=net)
    other = copy.deepcopy(FINETUNE_DATA_VAL)
    other["dataset"]["name"] = "CirImageList"
    with pytest.raises(NotImplementedError):
        initialize_validation(copy.deepcopy(FINETUNE_VALIDATION), data={"db": db, "images": images}, params_data={"val": other},
                              default_criterion=default, network=net)


def test_validate_stage_accepts_a_loader_section(monkeypatch):
    """stages.validate.validate with a ``data`` section: the loss validation runs; a ``data`` section nobody names is still refused"""
    import importlib
    V = importlib.import_module("gandtr_amd.stages.validate")
    monkeypatch.setattr(retrieval, "search_hard_negatives", _host_hard_negatives)
    monkeypatch.setattr(V, "load_network", lambda params, device: _MeanNet())
    gen = torch.Generator().manual_seed(6)
    images = [torch.randn(3, 8, 8, generator=gen) for _ in range(16)]
    db = {"qidxs": [0, 1, 2, 3], "pidxs": [4, 5, 6, 7], "cluster": list(range(8)) * 2}
    section = dict(copy.deepcopy(FINETUNE_VALIDATION), criterion=dict(FINETUNE_CRITERION))
    data_val = copy.deepcopy(FINETUNE_DATA_VAL)
    data_val["dataset"]["neg_num"] = 2
    out, = V.validate({"network": {}, "validation": section, "data": {"val": data_val}}, {"db": db, "images": images})
    keys = out["eval"]
    assert set(keys) == {"val/validation/loss:total_avg.4", "val/validation/data_mining:average_negative_distance_avg.4"}
    assert np.isfinite(keys["val/validation/loss:total_avg.4"]) and keys["val/validation/loss:total_avg.4"] >= 0
    with pytest.raises(NotImplementedError):
        V.validate({"network": {}, "validation": {}, "data": {"val": data_val}}, [images])
    score = {"type": "SingleValidation", "data": None, "criterion": {"type": "cirdatasetap"}, "network_overlay": None, "frequency": 1}
    with pytest.raises(NotImplementedError):
        V.validate({"network": {}, "validation": score, "data": {"val": data_val}}, [images])


def test_symbol_in_header_library_and_binding_and_argument_errors_without_a_gpu():
    """the argument checks of gdt_tuple_loss come first, so they run on a host without a GPU (the pointers are never read)"""
    from gandtr_amd import _hip
    header = open(os.path.join(ROOT, "include", "gandtr_hip.h")).read()
    for name in ("gdt_tuple_loss", "gdt_tuple_loss_workspace_bytes"):
        assert re.search(r"\bint %s\(" % name, header) and name in _hip.SIGNATURES
    assert "functional.py:141-157" in header and "validation.py:93-107" in header and "cirlosses.py" in header
    assert "tuple_loss.hip" in open(os.path.join(ROOT, "gandtr_amd", "csrc", "Makefile")).read()
    lib = _hip.load()
    assert hasattr(lib, "gdt_tuple_loss")
    need = ctypes.c_size_t()
    _hip.check(lib.gdt_tuple_loss_workspace_bytes(1700, 7, ctypes.byref(need)))
    assert need.value >= 1700 * 6 * 4
    for n_tuples, s in ((0, 7), (-1, 7), (10, 1), (10, 0)):
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_tuple_loss_workspace_bytes(n_tuples, s, ctypes.byref(need)))
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_tuple_loss_workspace_bytes(10, 7, None))
    p = 1 << 20                                                         # stands for a device address
    ok = dict(vecs=p, tuples=p, n_vec=100, d=37, n_tuples=10, s=7, kind=0, margin=0.75, eps=1e-6, pair=p, loss=p, total=p, ws=p, ws_bytes=10 * 6 * 4)
    for change in (dict(vecs=None), dict(tuples=None), dict(loss=None), dict(total=None), dict(ws=None), dict(n_vec=0), dict(d=0), dict(n_tuples=0),
                   dict(s=1), dict(kind=2), dict(kind=-1), dict(eps=-1.0), dict(margin=float("nan")), dict(ws_bytes=10 * 6 * 4 - 1), dict(ws_bytes=0),
                   dict(vecs=p + 2), dict(total=p + 4)):
        a = dict(ok, **change)
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_tuple_loss(a["vecs"], a["tuples"], a["n_vec"], a["d"], a["n_tuples"], a["s"], a["kind"], a["margin"], a["eps"], a["pair"],
                                          a["loss"], a["total"], a["ws"], a["ws_bytes"], None))
