"""mAP evaluation on the device: gdt_retrieval_average_precision against the reference's numbers (tests/golden/map_cases.npz) and the
numpy restatement, bit for bit; its status paths; and the ``validate`` stage end to end on a synthetic roxford5k-layout dataset
(JPEG files, bounding boxes, easy / hard / junk) plus a TSV dataset, with plain and multi-scale + whitened GeM-VGG16 networks."""
import contextlib
import copy
import io
import os
import pickle

import numpy as np
import pytest
import torch

from gandtr_amd.tools import synth

pytestmark = pytest.mark.gpu

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
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool(np.all(a[~np.isnan(a)] == b[~np.isnan(b)]))


@pytest.mark.parametrize("case", load_cases(), ids=lambda c: c[0])
def test_kernel_matches_the_reference_bit_for_bit(cuda_device, case):
    from gandtr_amd import retrieval
    name, proto, ranks, gnd, kappas, f = case
    rk = torch.from_numpy(ranks).to(cuda_device)
    if proto == "old":
        aps, prs = retrieval.average_precision(rk, [gnd], kappas)
        assert same(aps[0], f["aps"]) and same(prs[0], f["prs"])
        m, aps, pr, prs = retrieval.compute_map(rk, gnd, kappas)
        assert same(m, f["map"]) and same(aps, f["aps"]) and same(pr, f["pr"]) and same(prs, f["prs"])
    else:
        aps, prs = retrieval.average_precision(rk, retrieval._revisited_setups(gnd), kappas)
        for s, S in enumerate("EMH"):
            assert same(aps[s], f["aps_" + S]) and same(prs[s], f["prs_" + S])
        with contextlib.redirect_stdout(io.StringIO()) as text:
            avg, per = retrieval.compute_map_and_print("roxford5k", rk, gnd, kappas)
        assert text.getvalue() == str(f["printed"])
        for S, key in (("E", "easy"), ("M", "medium"), ("H", "hard")):
            assert same(avg["map_" + key], f["map_" + S]) and same(per["ap_" + key], f["aps_" + S])


def _random_gnd(rng, ndb, nq, big=None):
    gnd = []
    for q in range(nq):
        g = {k: rng.integers(-2, ndb + 2, int(rng.integers(0, n))).tolist() for k, n in (("easy", 120), ("hard", 80), ("junk", 200))}
        g["easy"].append(int(rng.integers(0, ndb)))                     # every easy list finds something: precision@k is defined
        g["hard"].append(int(rng.integers(0, ndb)))
        gnd.append(g)
    if big is not None:                                                 # one query with `big` positives
        gnd[big[0]]["easy"] = rng.choice(ndb, big[1], replace=False).tolist()
    return gnd


@pytest.mark.parametrize("ndb,nq,big", [(1000, 70, None), (5000, 7, (3, 5000)), (100000, 70, (11, 50000)), (200000, 70, None)])
def test_kernel_matches_numpy_on_random_ranks(cuda_device, ndb, nq, big):
    from gandtr_amd import retrieval
    rng = np.random.default_rng(ndb + nq)
    g = torch.Generator(device=cuda_device).manual_seed(ndb)
    rk = torch.argsort(torch.rand((nq, ndb), device=cuda_device, generator=g), dim=1).t()          # Ndb x Nq, a permutation per column
    host = rk.cpu().numpy().astype(np.int64)
    gnd = _random_gnd(rng, ndb, nq, big)
    setups = retrieval._revisited_setups(gnd)
    kappas = [1, 5, 10, 100]
    aps, prs = retrieval.average_precision(rk, setups, kappas)
    for s, setup in enumerate(setups):
        a, p = retrieval._map_host(host, setup, kappas)
        assert same(aps[s], a) and same(prs[s], p), s
    if big is not None:
        assert not np.isnan(aps[0][big[0]]) and len(set(gnd[big[0]]["easy"])) == big[1]


def test_status_paths(cuda_device):
    from gandtr_amd import retrieval
    ranks = torch.arange(6, device=cuda_device)[:, None].repeat(1, 2).int()
    gnd = [{"ok": [1], "junk": [0]}, {"ok": [2]}]
    dup = ranks.clone()
    dup[3, 1] = 0                                                       # a repeated index: not a permutation
    with pytest.raises(ValueError, match="permutation"):
        retrieval.average_precision(dup, [gnd], [1])
    out = ranks.clone()
    out[0, 0] = 6                                                       # an index outside the database
    with pytest.raises(ValueError, match="permutation"):
        retrieval.average_precision(out, [gnd], [])
    nothing = [{"ok": [9, -1]}, {"ok": [2]}]
    with pytest.raises(ValueError):                                     # positives, none found, kappas asked
        retrieval.average_precision(ranks, [nothing], [1])
    aps, prs = retrieval.average_precision(ranks, [nothing], [])
    assert aps[0, 0] == 0.0 and aps[0, 1] == (0.0 + 1.0 / 3) * 1.0 / 2.0 and prs.shape == (1, 2, 0)
    aps, _ = retrieval.average_precision(ranks, [gnd], [1])             # the same buffers run clean again after a refusal
    assert aps[0, 0] == 1.0


# ---- the validate stage end to end

SIZES = [(72, 96), (96, 72), (80, 80), (64, 104), (88, 64)]


def _jpeg(path, seed, hw):
    from PIL import Image
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.02, 0.2, (3, 2))
    ph = rng.uniform(0, 6.3, 3)
    img = np.stack([127 + 100 * np.sin(f[c, 0] * yy + f[c, 1] * xx + ph[c]) for c in range(3)], -1)
    img += rng.normal(0, 12, img.shape)
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8), "RGB").save(path, "JPEG", quality=90)


def _write_datasets(root, n=40):
    d = os.path.join(root, "data", "test", "roxford5k")
    os.makedirs(os.path.join(d, "jpg"))
    imlist = ["img_%02d" % i for i in range(n)]
    for i, name in enumerate(imlist):
        _jpeg(os.path.join(d, "jpg", name + ".jpg"), i, SIZES[i % len(SIZES)])
    h0, w0 = SIZES[0]
    gnd = [{"easy": [0], "hard": [], "junk": [], "bbx": [0, 0, w0, h0]},                # the whole image: ap_easy == 1
           {"easy": [5, 6], "hard": [7], "junk": [8], "bbx": [4, 6, 60, 50]},
           {"easy": [], "hard": [10, 11], "junk": [12], "bbx": [10, 0, 70, 64]},          # no easy positive: NaN, excluded
           {"easy": [15, 1, 2], "hard": [3], "junk": [15, 16], "bbx": [0, 8, 64, 72]}]
    with open(os.path.join(d, "gnd_roxford5k.pkl"), "wb") as f:
        pickle.dump({"imlist": imlist, "qimlist": [imlist[0], imlist[5], imlist[10], imlist[15]], "gnd": gnd}, f)
    db, qs = os.path.join(root, "db.tsv"), os.path.join(root, "queries.tsv")
    with open(db, "w") as f:
        f.write("identifier\n" + "".join(x + "\n" for x in imlist))
    with open(qs, "w") as f:                                           # old protocol: each query's only positive is its own image
        f.write("query\tbbx\tok\tjunk\n" + "".join('%s\t\t["%s"]\t[]\n' % (x, x) for x in (imlist[20], imlist[33])))
    tsv = {"name": "selfset", "queries": qs, "db": db, "imgdir": os.path.join(d, "jpg")}
    return d, imlist, gnd, tsv


def _checkpoint(tmp_path):
    import hubconf
    base = hubconf.gem_vgg16_cyclegan(pretrained=False, device="cpu")
    base.model.load_state_dict(synth.vgg16_state(0))
    sd = base.state_dict()["net"]
    sd["network_params"]["runtime"]["data"] = {"transforms": "pil2np | totensor | normalize",
                                               "mean_std": [[0.485, 0.456, 0.406], [0.229, 0.224, 0.225]]}
    ck, lw = str(tmp_path / "vgg.pth"), str(tmp_path / "lw.pkl")
    torch.save(sd, ck)
    with open(lw, "wb") as f:
        pickle.dump(synth.whitening_state(0, 512), f)
    return ck, lw


def test_validate_stage_end_to_end(cuda_device, tmp_path, monkeypatch):
    from gandtr_amd import retrieval
    from gandtr_amd.datasets import ImagesFromList
    from gandtr_amd.learning import load_network
    from gandtr_amd.stages import FUNCTIONS
    from gandtr_amd.stages.validate import extract_vectors, extract_vectors_from_files
    validate = FUNCTIONS["mdir.stages.validate.validate"]
    d, imlist, gnd, tsv = _write_datasets(str(tmp_path))
    monkeypatch.setenv("CIRTORCH_ROOT", str(tmp_path))
    ck, lw = _checkpoint(tmp_path)
    size = 96
    task = lambda ds: {"type": "SingleValidation", "frequency": None, "network_overlay": None, "data": None,   # noqa: E731
                       "criterion": {"type": "cirdatasetap", "image_size": size, "dataset": ds}}
    validation = {"type": "MultiCriterialValidation", "decisive_criterion": None, "roxford5k": task("roxford5k"), "selfset": task(tsv)}
    for wrappers in ("cirfaketuplebatch",
                     {"train": None, "eval": {"0_cirwhiten": {"whitening": lw, "dimensions": None}, "1_cirmultiscale": {"scales": True}}}):
        network = {"path": ck, "runtime": {"wrappers": wrappers}}
        out = validate({"network": copy.deepcopy(network), "validation": copy.deepcopy(validation), "data": {}}, ())
        assert isinstance(out, tuple) and len(out) == 1 and set(out[0]) == {"eval"}
        ev = out[0]["eval"]
        rox = "roxford5k/validation/"
        assert set(ev) == {rox + "score_avg:map_easy", rox + "score_avg:map_medium", rox + "score_avg:map_hard",
                           rox + "score:ap_easy_avg.4", rox + "score:ap_medium_avg.4", rox + "score:ap_hard_avg.4",
                           "selfset/validation/score_avg:map", "selfset/validation/score:ap_avg.4"}
        # known answers: a query that is its whole database image, with that image its only positive, ranks it first
        assert ev["selfset/validation/score_avg:map"] == 1.0 and ev["selfset/validation/score:ap_avg.4"] == 1.0
        # the same files through the plain device path, evaluated by the numpy restatement: the same numbers
        net = load_network(copy.deepcopy(network), cuda_device).eval()
        mean_std = net.network_params.runtime["data"]["mean_std"]
        files = [os.path.join(d, "jpg", x + ".jpg") for x in imlist]
        with torch.no_grad():
            vecs = extract_vectors_from_files(net, files, size, mean_std, cuda_device)
            qfiles = [files[i] for i in (0, 5, 10, 15)]
            qdata = ImagesFromList("", qfiles, imsize=size, bbxs=[tuple(g["bbx"]) for g in gnd], transform=mean_std, device=cuda_device)
            qvecs = extract_vectors(net, qdata.batch(range(4)), cuda_device, batched=True)
        _, ranks = retrieval.scores_and_ranks(vecs, qvecs)
        with contextlib.redirect_stdout(io.StringIO()):
            avg, per = retrieval.compute_map_and_print("roxford5k", ranks.cpu().numpy().astype(np.int64), gnd)
        assert per["ap_easy"][0] == 1.0 and np.isnan(per["ap_easy"][2])
        for key in ("easy", "medium", "hard"):
            assert ev[rox + "score_avg:map_" + key] == avg["map_" + key], key
            assert ev[rox + "score:ap_%s_avg.4" % key] == float(np.nanmean(per["ap_" + key])), key
