"""Generates tests/golden/map_cases.npz by running the reference's own compute_map / compute_map_and_print
(mdir/external/cirtorch/utils/evaluate.py, loaded by path: it needs only numpy) on crafted ranks and ground truth.
Run in the build container:  python tests/golden/make_map_golden.py

Per case ``<name>/...``: ``ranks`` (Ndb x Nq; the random cases store only ``hash`` = (ndb, nq, seed) and rebuild them with
``hashed_ranks``), ``kappas``, the ground-truth lists as CSR (``<list>_off`` / ``<list>_ids``; old protocol: ok, junk and ``has_junk`` per
query -- 0 where the dict has no "junk" key; revisited protocol: easy, hard, junk) and the reference's results: old protocol
``map, aps, pr, prs`` of compute_map(ranks, gnd, kappas); revisited protocol ``map_<S>, aps_<S>, pr_<S>, prs_<S>`` of compute_map on the
setups S = E / M / H of evaluate.py:118-140.  ``names`` lists the cases, ``protocol`` says which form each one has."""
import contextlib
import importlib.util
import io
import os

import numpy as np

REF = "/root/reference/mdir/external/cirtorch/utils/evaluate.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "map_cases.npz")


def hashed_ranks(ndb, nq, seed):
    """a deterministic Ndb x Nq permutation matrix without an RNG stream: argsort of an integer hash per column"""
    i = np.arange(ndb, dtype=np.uint64)[:, None]
    q = np.arange(nq, dtype=np.uint64)[None, :]
    h = (i * np.uint64(2654435761) + q * np.uint64(40503) + np.uint64(seed) * np.uint64(97)) % np.uint64(4294967291)
    h = (h * np.uint64(2246822519)) % np.uint64(4294967279)
    return np.argsort(h, axis=0, kind="stable")


def csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    ids = np.concatenate([np.asarray(x, dtype=np.int64).reshape(-1) for x in lists]) if lists else np.zeros(0, np.int64)
    return off, ids.astype(np.int64)


def perm_cols(rng, ndb, nq):
    return np.stack([rng.permutation(ndb) for _ in range(nq)], axis=1)


def old_cases(rng):
    """(name, ranks, gnd, kappas): every edge the kernel has to get right"""
    r = np.arange(10)[:, None]
    c = []
    c.append(("basic", perm_cols(rng, 10, 3), [{"ok": [1, 4], "junk": [7]}, {"ok": [0, 2, 9], "junk": [3, 5]}, {"ok": [6], "junk": []}], [1, 2, 5]))
    c.append(("duplicates", perm_cols(rng, 12, 2), [{"ok": [3, 3, 5, 5, 5], "junk": [1, 1]}, {"ok": [0, 11, 0], "junk": [11]}], [1, 3]))
    c.append(("pos_also_junk", np.tile(r, (1, 3)), [{"ok": [2, 3], "junk": [2]}, {"ok": [0, 1], "junk": [0]}, {"ok": [4, 6, 8], "junk": [6, 5]}], [1, 2, 10]))
    c.append(("empty_ok", perm_cols(rng, 10, 3), [{"ok": [], "junk": [1]}, {"ok": [2, 5], "junk": [0]}, {"ok": [], "junk": []}], [1, 5]))
    c.append(("missing_junk", perm_cols(rng, 10, 2), [{"ok": [3, 8]}, {"ok": [1], "junk": [2]}], [1, 5]))
    c.append(("junk_around", np.tile(r, (1, 3)), [{"ok": [3, 6], "junk": [0, 1]}, {"ok": [2, 7], "junk": [4, 5]}, {"ok": [1, 2], "junk": [8, 9]}],
              [1, 2, 3]))
    c.append(("pos_rank0", np.tile(r, (1, 2)), [{"ok": [0], "junk": []}, {"ok": [0, 1, 2], "junk": [5]}], [1, 5]))
    c.append(("kappa_large", perm_cols(rng, 10, 2), [{"ok": [1, 2], "junk": [3]}, {"ok": [9], "junk": []}], [5, 100, 1000]))
    c.append(("out_of_range", perm_cols(rng, 10, 3), [{"ok": [-1, 4, 10, 99], "junk": [-5, 12, 2]}, {"ok": [5, 2 ** 31 - 1], "junk": []},
                                                      {"ok": [0, 1, -2], "junk": [10]}], [1, 2]))
    c.append(("one_image_db", np.zeros((1, 2), dtype=np.int64), [{"ok": [0], "junk": []}, {"ok": [0, 0, 3], "junk": [0]}], [1, 5]))
    c.append(("all_positive", perm_cols(rng, 40, 2), [{"ok": list(range(40)), "junk": []}, {"ok": list(range(39, -1, -1)), "junk": [5, 6]}], [1, 5, 10, 40]))
    c.append(("nothing_found", perm_cols(rng, 8, 2), [{"ok": [-1, 8], "junk": [1]}, {"ok": [3], "junk": []}], []))
    c.append(("junk_only_before", np.tile(r, (1, 1)), [{"ok": [9], "junk": list(range(9))}], [1, 5]))
    c.append(("ties_after_junk", np.tile(r, (1, 2)), [{"ok": [1, 2, 3], "junk": [1, 2]}, {"ok": [0, 1, 2, 3], "junk": [0, 1, 2]}], [1, 2]))
    for s in range(4):
        ndb, nq = 5000, 70
        ranks = hashed_ranks(ndb, nq, s)
        gnd = []
        for q in range(nq):
            n_ok = int(rng.integers(0, 60)) if q % 17 else 0
            g = {"ok": rng.integers(-3, ndb + 3, n_ok).tolist()}
            if q % 5:
                g["junk"] = rng.integers(0, ndb, int(rng.integers(0, 30))).tolist()
            gnd.append(g)
        for g in gnd:                                 # every non-empty list holds an in-range id: precision@k is defined
            if g["ok"] and not any(0 <= x < ndb for x in g["ok"]):
                g["ok"].append(int(rng.integers(0, ndb)))
        c.append(("random_old_%d" % s, (ndb, nq, s), gnd, [1, 5, 10]))
    return c


def new_cases(rng):
    c = []
    r = np.arange(12)[:, None]
    c.append(("rox_small", np.tile(r, (1, 3)), [{"easy": [0, 4], "hard": [2, 7], "junk": [1]}, {"easy": [5], "hard": [], "junk": [0, 3]},
                                                {"easy": [3, 3, 11], "hard": [3], "junk": [11]}], [1, 5, 10]))
    c.append(("rox_perm", perm_cols(rng, 30, 4), [{"easy": [1, 2, 3], "hard": [10, 20], "junk": [4, 5, 29]}, {"easy": [7], "hard": [8, 9], "junk": []},
                                                  {"easy": [0, 29], "hard": [15], "junk": [14, 16, 40]}, {"easy": [12], "hard": [13], "junk": [-1]}], [1, 5, 10]))
    for s in range(4):
        ndb, nq = 5000, 70
        gnd = []
        for q in range(nq):
            g = {k: rng.integers(0, ndb, int(rng.integers(1, n))).tolist() for k, n in (("easy", 40), ("hard", 40), ("junk", 60))}
            gnd.append(g)
        c.append(("random_new_%d" % s, (ndb, nq, 10 + s), gnd, [1, 5, 10]))
    return c


def main():
    spec = importlib.util.spec_from_file_location("ref_evaluate", REF)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(0)
    out, names, protocol = {}, [], []
    for name, ranks, gnd, kappas in old_cases(rng):
        if isinstance(ranks, tuple):
            out[name + "/hash"] = np.array(ranks)
            ranks = hashed_ranks(*ranks)
        else:
            out[name + "/ranks"] = ranks.astype(np.int32)
        out[name + "/kappas"] = np.array(kappas, dtype=np.int64)
        for k in ("ok", "junk"):
            out[name + "/%s_off" % k], out[name + "/%s_ids" % k] = csr([g.get(k, []) for g in gnd])
        out[name + "/has_junk"] = np.array([int("junk" in g) for g in gnd])
        m, aps, pr, prs = ref.compute_map(ranks, gnd, kappas)
        out.update({name + "/map": np.float64(m), name + "/aps": aps, name + "/pr": pr, name + "/prs": prs})
        names.append(name)
        protocol.append("old")
    for name, ranks, gnd, kappas in new_cases(rng):
        if isinstance(ranks, tuple):
            out[name + "/hash"] = np.array(ranks)
            ranks = hashed_ranks(*ranks)
        else:
            out[name + "/ranks"] = ranks.astype(np.int32)
        out[name + "/kappas"] = np.array(kappas, dtype=np.int64)
        for k in ("easy", "hard", "junk"):
            out[name + "/%s_off" % k], out[name + "/%s_ids" % k] = csr([g[k] for g in gnd])
        # the setups of evaluate.py:118-140
        setups = {"E": [{"ok": np.concatenate([g["easy"]]), "junk": np.concatenate([g["junk"], g["hard"]])} for g in gnd],
                  "M": [{"ok": np.concatenate([g["easy"], g["hard"]]), "junk": np.concatenate([g["junk"]])} for g in gnd],
                  "H": [{"ok": np.concatenate([g["hard"]]), "junk": np.concatenate([g["junk"], g["easy"]])} for g in gnd]}
        for s, g in setups.items():
            m, aps, pr, prs = ref.compute_map(ranks, g, kappas)
            out.update({name + "/map_" + s: np.float64(m), name + "/aps_" + s: aps, name + "/pr_" + s: pr, name + "/prs_" + s: prs})
        with contextlib.redirect_stdout(io.StringIO()) as text:
            avg, per = ref.compute_map_and_print("roxford5k", ranks, gnd, kappas)
        out[name + "/printed"] = np.array(text.getvalue())
        assert avg["map_easy"] == out[name + "/map_E"] and np.array_equal(per["ap_hard"], out[name + "/aps_H"], equal_nan=True)
        names.append(name)
        protocol.append("new")
    out["names"] = np.array(names)
    out["protocol"] = np.array(protocol)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, len(names), "cases", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
