"""mAP evaluation without a GPU: the numpy ``compute_map`` / ``compute_map_and_print`` against the reference's own numbers
(tests/golden/map_cases.npz, made by tests/golden/make_map_golden.py), the two dataset forms of ``CirDatasetAp``, the validation schema
and its errors, the metadata keys of the ``validate`` stage, and the argument checks of the C entry point (before any HIP call)."""
import contextlib
import ctypes
import io
import json
import os
import pickle

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "map_cases.npz")


def hashed_ranks(ndb, nq, seed):
    """the generator's deterministic rank matrix (tests/golden/make_map_golden.py)"""
    i = np.arange(ndb, dtype=np.uint64)[:, None]
    q = np.arange(nq, dtype=np.uint64)[None, :]
    h = (i * np.uint64(2654435761) + q * np.uint64(40503) + np.uint64(seed) * np.uint64(97)) % np.uint64(4294967291)
    h = (h * np.uint64(2246822519)) % np.uint64(4294967279)
    return np.argsort(h, axis=0, kind="stable")


def load_cases():
    g = np.load(GOLDEN)
    cases = []
    for name, proto in zip(g["names"], g["protocol"]):
        name, proto = str(name), str(proto)
        f = {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith(name + "/")}
        ranks = hashed_ranks(*[int(v) for v in f["hash"]]) if "hash" in f else f["ranks"].astype(np.int64)
        lists = ("ok", "junk") if proto == "old" else ("easy", "hard", "junk")
        cols = {k: [f[k + "_ids"][f[k + "_off"][i]:f[k + "_off"][i + 1]].tolist() for i in range(ranks.shape[1])] for k in lists}
        if proto == "old":
            gnd = [{"ok": ok} if not hj else {"ok": ok, "junk": jk} for ok, jk, hj in zip(cols["ok"], cols["junk"], f["has_junk"])]
        else:
            gnd = [{"easy": e, "hard": h, "junk": j} for e, h, j in zip(cols["easy"], cols["hard"], cols["junk"])]
        cases.append((name, proto, ranks, gnd, [int(k) for k in f["kappas"]], f))
    return cases


def same(a, b):
    """== on every float, NaN where the reference has NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool(np.all(a[~np.isnan(a)] == b[~np.isnan(b)]))


def test_fixture_covers_the_edges():
    names = {c[0] for c in load_cases()}
    assert len(names) >= 20
    assert {"duplicates", "pos_also_junk", "empty_ok", "missing_junk", "junk_around", "pos_rank0", "kappa_large", "out_of_range",
            "one_image_db", "all_positive", "nothing_found", "rox_small"} <= names


@pytest.mark.parametrize("case", load_cases(), ids=lambda c: c[0])
def test_numpy_compute_map_matches_the_reference_bit_for_bit(case):
    from gandtr_amd import retrieval
    name, proto, ranks, gnd, kappas, f = case
    if proto == "old":
        m, aps, pr, prs = retrieval.compute_map(ranks, gnd, kappas)
        assert same(m, f["map"]) and same(aps, f["aps"]) and same(pr, f["pr"]) and same(prs, f["prs"])
        with contextlib.redirect_stdout(io.StringIO()) as text:
            avg, per = retrieval.compute_map_and_print(name, ranks, gnd)
        assert set(avg) == {"map"} and set(per) == {"ap"}
        m0, aps0, _, _ = retrieval.compute_map(ranks, gnd)
        assert same(avg["map"], m0) and same(per["ap"], aps0) and same(aps0, f["aps"])
        assert text.getvalue() == ">> {}: mAP {:.2f}\n".format(name, np.around(m0 * 100, decimals=2))
    else:
        with contextlib.redirect_stdout(io.StringIO()) as text:
            avg, per = retrieval.compute_map_and_print("roxford5k", ranks, gnd, kappas)
        assert text.getvalue() == str(f["printed"])
        for s, key in (("E", "easy"), ("M", "medium"), ("H", "hard")):
            assert same(avg["map_" + key], f["map_" + s]) and same(per["ap_" + key], f["aps_" + s])
        for s, setup in zip("EMH", retrieval._revisited_setups(gnd)):
            m, aps, pr, prs = retrieval.compute_map(ranks, setup, kappas)
            assert same(m, f["map_" + s]) and same(aps, f["aps_" + s]) and same(pr, f["pr_" + s]) and same(prs, f["prs_" + s])


def test_numpy_compute_map_edges():
    from gandtr_amd import retrieval
    ranks = np.arange(6)[:, None].repeat(2, 1)
    with pytest.raises(ValueError):                                   # positives, none found, kappas asked: the reference's max() raises
        retrieval.compute_map(ranks, [{"ok": [7]}, {"ok": [1]}], [1])
    m, aps, pr, prs = retrieval.compute_map(ranks, [{"ok": []}, {"ok": []}], [1, 5])
    assert np.isnan(m) and np.isnan(aps).all() and np.isnan(pr).all()   # every query empty: NaN
    assert retrieval.compute_map_and_print("tokyo", ranks, [{"easy": [1], "hard": [], "junk": []}] * 2) is None


def _write_rox(root, n=6):
    d = os.path.join(root, "data", "test", "roxford5k")
    os.makedirs(os.path.join(d, "jpg"))
    imlist = ["img_%02d" % i for i in range(n)]
    gnd = [{"easy": [0], "hard": [2], "junk": [1], "bbx": [0.0, 0.0, 10.0, 12.0]},
           {"easy": [3, 4], "hard": [], "junk": [], "bbx": None}]
    with open(os.path.join(d, "gnd_roxford5k.pkl"), "wb") as f:
        pickle.dump({"imlist": imlist, "qimlist": [imlist[0], imlist[5]], "gnd": gnd}, f)
    return d, imlist, gnd


def _spec(dataset):
    return {"type": "cirdatasetap", "image_size": 64, "dataset": dataset, "transforms": "pil2np | totensor | normalize",
            "mean_std": [[0.5] * 3, [0.5] * 3]}


def test_cirdatasetap_named_dataset_form(tmp_path, monkeypatch):
    from gandtr_amd.components.optim.score import initialize_score
    d, imlist, gnd = _write_rox(str(tmp_path))
    monkeypatch.setenv("CIRTORCH_ROOT", str(tmp_path))
    score = initialize_score(_spec("roxford5k"))
    assert score.images == [os.path.join(d, "jpg", x + ".jpg") for x in imlist]
    assert score.qimages == [os.path.join(d, "jpg", imlist[0] + ".jpg"), os.path.join(d, "jpg", imlist[5] + ".jpg")]
    assert score.bbxs == [(0.0, 0.0, 10.0, 12.0), None] and score.gnd == gnd and score.dataset == "roxford5k"
    assert score.decisive_criterion == "val/learning/score_avg:map_medium"
    with pytest.raises(ValueError):
        initialize_score(_spec("notadataset"))
    monkeypatch.delenv("CIRTORCH_ROOT")
    with pytest.raises(ValueError):
        initialize_score(_spec("roxford5k"))
    with pytest.raises(ValueError):                                   # the device path: no CPU evaluation
        monkeypatch.setenv("CIRTORCH_ROOT", str(tmp_path))
        initialize_score(_spec("roxford5k"))(None, "cpu", lambda *a: None)


def test_cirdatasetap_tsv_form(tmp_path):
    from gandtr_amd.components.optim.score import initialize_score
    db, qs = str(tmp_path / "db.tsv"), str(tmp_path / "queries.tsv")
    with open(db, "w") as f:
        f.write("identifier\tother\n" + "".join("a/%d\tx\n" % i for i in range(4)) + "b/z.png\tx\n")
    with open(qs, "w") as f:
        f.write("query\tbbx\tok\tjunk\n")
        f.write("a/0\t[1, 2, 30, 40]\t%s\t%s\n" % (json.dumps(["a/0", "a/2"]), json.dumps(["a/1"])))
        f.write("q/extra\t\t%s\t[]\n" % json.dumps(["b/z.png"]))
    spec = _spec({"name": "tsvset", "queries": qs, "db": db, "imgdir": "/imgs"})
    score = initialize_score(spec)
    assert score.dataset == "tsvset"
    assert score.images == ["/imgs/a/0.jpg", "/imgs/a/1.jpg", "/imgs/a/2.jpg", "/imgs/a/3.jpg", "/imgs/b/z.png"]
    assert score.qimages == ["/imgs/a/0.jpg", "/imgs/q/extra.jpg"]
    assert score.bbxs == [(1, 2, 30, 40), None]
    assert score.gnd == [{"ok": [0, 2], "junk": [1]}, {"ok": [4], "junk": []}]
    with pytest.raises(ValueError):
        initialize_score(_spec({"name": "x", "queries": qs, "db": db}))


def test_validation_schema_and_errors(tmp_path, monkeypatch):
    import copy
    from gandtr_amd.components.optim.score import SCORES, initialize_score
    from gandtr_amd.learning import validation as V
    import mdir
    import mdir.learning.validation
    import mdir.components.optim.score
    assert mdir.learning.validation.initialize_validation is V.initialize_validation
    assert mdir.components.optim.score.SCORES is SCORES and set(SCORES) == {"cirdatasetap"}
    with pytest.raises(NotImplementedError):
        initialize_score({"type": "visual"})
    with pytest.raises(NotImplementedError):
        initialize_score({"type": "nosuchscore"})
    with pytest.raises(NotImplementedError):
        V.initialize_validation({"type": "cirtorch", "dataset": "roxford5k"})
    assert isinstance(V.initialize_validation(False), V.NoValidation) and V.initialize_validation("x").decisive_criterion == "x"

    class Net:
        network_params = type("P", (), {"runtime": {"data": {"transforms": "pil2np | totensor | normalize", "mean_std": [[0.5] * 3, [0.5] * 3]}}})()
    _write_rox(str(tmp_path))
    monkeypatch.setenv("CIRTORCH_ROOT", str(tmp_path))
    single = {"type": "SingleValidation", "frequency": 2, "criterion": {"type": "cirdatasetap", "image_size": 64, "dataset": "roxford5k"},
              "network_overlay": None, "data": None}
    with pytest.raises(NotImplementedError):
        V.initialize_validation({**copy.deepcopy(single), "data": "val"}, network=Net())
    with pytest.raises(ValueError):
        V.initialize_validation({**copy.deepcopy(single), "criterion": "default"}, network=Net(), default_criterion=None)
    sv = V.initialize_validation(copy.deepcopy(single), network=Net())
    assert sv.decisive_criterion == "val/learning/score_avg:map_medium" and sv.criterion.image_size == 64
    assert [k for k, _ in sv.validations(None)] == ["val"] and sv.validations(0) == [] and len(sv.validations(1)) == 1
    multi = V.initialize_validation({"type": "MultiCriterialValidation", "decisive_criterion": None, "roxford5k": copy.deepcopy(single),
                                     "rox2": {**copy.deepcopy(single), "frequency": None}}, network=Net())
    assert [k for k, _ in multi.validations(None)] == ["roxford5k", "rox2"] and [k for k, _ in multi.validations(1)] == ["roxford5k"]


def test_validate_stage_metadata_keys():
    """the keys the reference's MetadataKeeper makes of the rows CirDatasetAp logs (mdir/tools/eventprocessor.py:75-121)"""
    from gandtr_amd.stages.validate import _ValidationMetadata
    ev = _ValidationMetadata()
    log = ev.logger("roxford5k")
    log(None, 3, "dataset", {"extract_descriptors": 1.0}, "scalar/time")
    log(None, 3, "score_avg", {"map_easy": 0.5, "map_medium": 0.25, "map_hard": 0.125}, "scalar/score")
    for i, (e, m) in enumerate([(0.5, 1.0), (np.nan, 0.5), (0.25, 0.0)]):
        log(i, 3, "score", {"ap_easy": e, "ap_medium": m}, "scalar/score")
    old = ev.logger("tokyo")
    old(None, 1, "score_avg", {"map": 0.75}, "scalar/score")
    old(0, 1, "score", {"ap": 0.75}, "scalar/score")
    assert ev.metadata() == {"roxford5k/validation/score_avg:map_easy": 0.5, "roxford5k/validation/score_avg:map_medium": 0.25,
                             "roxford5k/validation/score_avg:map_hard": 0.125, "roxford5k/validation/score:ap_easy_avg.4": 0.375,
                             "roxford5k/validation/score:ap_medium_avg.4": 0.5, "tokyo/validation/score_avg:map": 0.75,
                             "tokyo/validation/score:ap_avg.4": 0.75}


def _ap_call(lib, ranks, ndb, nq, nsetups, ok_off, junk_off, kappas, nk):
    ip = ctypes.POINTER(ctypes.c_int)
    arr = lambda v: (ctypes.c_int * len(v))(*v)                        # noqa: E731
    return lib.gdt_retrieval_average_precision(ranks, ndb, nq, nsetups, None, None, None, None, ctypes.cast(arr(ok_off), ip),
                                               ctypes.cast(arr(junk_off), ip), arr(kappas or [0]), nk, None, None, None, None, 0, None)


def test_average_precision_abi_checks_arguments_without_gpu():
    from gandtr_amd import _hip
    lib = _hip.load()
    bytes_ = ctypes.c_size_t()
    _hip.check(lib.gdt_retrieval_ap_workspace_bytes(100, 3, 3, 10, ctypes.byref(bytes_)))
    assert bytes_.value >= 3 * 100 * 4
    for args in [(0, 3, 3, 10), (100, 0, 3, 10), (100, 3, 0, 10), (100, 3, 3, -1), (1 << 16, 1 << 15, 1, 0)]:
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_retrieval_ap_workspace_bytes(*args, ctypes.byref(bytes_)))
    z = [0] * 4
    bad = [
        (None, 0, 3, 1, z, z, [1], 1),                                 # ndb < 1
        (None, 10, 3, 1, [0, 2, 1, 3], z, [1], 1),                     # offsets decrease
        (None, 10, 3, 1, [1, 2, 3, 4], z, [1], 1),                     # offsets do not start at 0
        (None, 10, 3, 1, z, [0, 0, 5, 4], [1], 1),                     # junk offsets decrease
        (None, 10, 3, 1, z, z, [1] * 17, 17),                          # more than 16 kappas
        (None, 10, 3, 1, z, z, [0], 1),                                # kappa < 1
        (None, 10, 3, 1, z, z, [1], -1),
        (None, 1 << 16, 1 << 15, 1, [0] * ((1 << 15) + 1), [0] * ((1 << 15) + 1), [1], 1),   # ndb * nq >= 2^31
    ]
    for args in bad:
        with pytest.raises(ValueError):
            _hip.check(_ap_call(lib, *args))
    with pytest.raises(ValueError):                                    # valid sizes, null device buffers: refused before any HIP call
        _hip.check(_ap_call(lib, None, 10, 3, 1, z, z, [1], 1))
