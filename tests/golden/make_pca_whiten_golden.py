"""Generates tests/golden/pca_whiten.npz by running the reference's own code on small synthetic descriptor sets (build container only):
    pcawhitenlearn                                          mdir/external/cirtorch/utils/whiten.py, loaded by path like make_whiten_golden.py
    learn_pca_whitening, paste_pca_normalize, l2_normalize  mdir/stages/whiten.py, imported with make_golden's placeholders
The npz holds arrays only.  Inputs are float32 (stored for the PCA cases, regenerated from the seed by tests/pca_whiten_ref.py for the paste
cases); the last paste case (no `dimensions`: every row is normalised on its own) stores every 4th output row to stay under the size limit.
Prints, per case, the two quantities the tests' gates rest on: the agreement of the reference (np.linalg.eig) with the eigh restatement, and the
relative eigengap at `dimensions`.  A case is kept only when both are at least 10x inside the gates (1e-8 / 1e-10); otherwise change the seed.
python tests/golden/make_pca_whiten_golden.py"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import make_golden              # noqa: E402
import pca_whiten_ref as R      # noqa: E402

REF = make_golden.REF


def main():
    spec = importlib.util.spec_from_file_location("ref_whiten", os.path.join(REF, "mdir/external/cirtorch/utils/whiten.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    make_golden._install_placeholders()
    sys.path.insert(0, REF)
    for name in [k for k in sys.modules if k == "mdir" or k.startswith("mdir.")]:
        del sys.modules[name]
    import mdir.stages.whiten as stage
    assert stage.__file__.startswith(REF), stage.__file__

    out = {}
    for i, (d, n, shrink) in enumerate(R.PCA_CASES):
        X32 = R.descriptors(i, d, n).T.copy()                                   # D x N
        X = X32.astype(np.float64)
        m, P = ref.pcawhitenlearn(X, shrink)
        meta, learned = stage.learn_pca_whitening({"shrink": shrink}, (X32.T.copy(),))
        assert np.array_equal(learned["P"], P) and np.array_equal(learned["m"], m)          # the stage is the function on values.astype(float64).T
        m2, P2, eig, shrunk = R.pcawhitenlearn(X, shrink)
        unit = P.real * np.sqrt(shrunk)[:, None]
        agree = R.rows_up_to_sign_abs(unit, P2 * np.sqrt(shrunk)[:, None])
        norms = np.abs(np.linalg.norm(P.real, axis=1) * np.sqrt(shrunk) - 1).max()
        print("pca case %d (d %d, n %d, shrink %s): unit rows eig vs eigh %.2e (gate 1e-8), row norms vs eigenvalues %.2e, cond %.1e"
              % (i, d, n, shrink, agree, norms, eig[0] / eig[-1]))
        assert np.isrealobj(P) and agree < 1e-9 and norms < 1e-9
        out.update({"pca_X_%d" % i: X32, "pca_m_%d" % i: m, "pca_P_%d" % i: P, "pca_eig_%d" % i: eig})
    for j, (d1, d2, n, dims) in enumerate(R.PASTE_CASES):
        a, b = R.paste_inputs(j)
        meta, value = stage.paste_pca_normalize({"dimensions": dims}, (a.astype(np.float64), b.astype(np.float64)))
        mine = R.paste_pca_normalize((a, b), dims)
        if dims:
            cat = np.concatenate([a, b], axis=1).astype(np.float64)
            cat -= cat.mean()
            w = np.linalg.eigvalsh(cat.T @ cat)[::-1]
            gap = (w[dims - 1] - w[dims]) / w[0]
            bound = (d1 + d2) * 2.0 ** -52 / gap
            print("paste case %d (%d+%d, n %d, dims %d): relative eigengap %.2e, bound D eps / gap %.2e, eig vs eigh %.2e (gate 1e-10)"
                  % (j, d1, d2, n, dims, gap, bound, np.abs(value - mine).max()))
            assert np.isrealobj(value) and bound < 1e-11 and np.abs(value - mine).max() < 1e-11
            out["paste_out_%d" % j] = value
        else:
            assert meta == {}
            print("paste case %d (%d+%d, n %d, no dimensions): restatement differs by %.2e" % (j, d1, d2, n, np.abs(value - mine).max()))
            out["paste_out_%d" % j] = value[::R.PASTE_STORED_ROWS].copy()
    # l2_normalize on the first paste case's left half
    a, _ = R.paste_inputs(0)
    meta, value = stage.l2_normalize({}, (3.0 * a.astype(np.float64),))
    assert meta == {}
    out["l2n_out"] = value
    path = os.path.join(HERE, "pca_whiten.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
