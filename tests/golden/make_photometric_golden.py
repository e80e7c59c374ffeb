"""Generate tests/golden/photometric.npz by IMPORTING THE REFERENCE's transform/functional.py (read-only) -- the way make_gan_data_golden.py does.

Runs only where the reference is present.  The module is loaded alone, by its directory as a package, with a placeholder ``cv2`` (it is imported at the top
and not used by the channel functions).  ``functional.py`` calls ``scipy.optimize.newton`` without importing scipy: the module's ``scipy`` attribute is set
to a shim whose ``optimize.newton`` calls the real one and records the exponent it returns.  The three channel functions then run unchanged.

The cases and the seeded input planes live in tests/photometric_ref.py.  The file holds: ``histogram_<name>`` (the reference's three named targets, the
keys ``gandtr_amd.photometric.load_histograms`` reads), and per case ``<kind>_<h>x<w>_match_<histogram>``, ``_c2c`` (matched to the plane
``photometric_ref.other_plane()``), ``_gamma_<target>`` (the output, cast to float32) and ``_gammas`` (float64: the clipped exponent per target, in the order
of the case's targets).

usage:  python tests/golden/make_photometric_golden.py
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import photometric_ref as R                                   # noqa: E402

REF_TRANSFORM = "/root/reference/mdir/components/data/transform"


def load_functional():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    pkg = types.ModuleType("ref_transform")
    pkg.__path__ = [REF_TRANSFORM]
    sys.modules["ref_transform"] = pkg
    return importlib.import_module("ref_transform.functional")


def main():
    import scipy.optimize
    func = load_functional()
    found = []

    def newton(*args, **kwargs):
        found.append(scipy.optimize.newton(*args, **kwargs))
        return found[-1]
    func.scipy = types.SimpleNamespace(optimize=types.SimpleNamespace(newton=newton))

    arrays = {"histogram_" + name: np.asarray(func.HISTOGRAMS[name], dtype=np.float64) for name in R.NAMES}
    other = R.other_plane()
    for kind, shape, histograms, c2c, targets in R.cases():
        chan = R.plane(kind, *shape)
        for hist in histograms:
            arrays[R.key(kind, shape, "match_" + hist)] = func.channel_histogram_matching(chan.copy(), hist)
        if c2c:
            arrays[R.key(kind, shape, "c2c")] = func.channel2channel_histogram_matching(chan.copy(), other.copy())
        gammas = []
        for target in targets:
            del found[:]
            out = func.channel_gamma_matching(chan.copy(), target)
            assert np.isfinite(out).all(), (kind, shape, target)
            # the exponent applied: newton's result clipped, or the fall-back after its RuntimeError (then nothing was recorded)
            with np.errstate(all="ignore"):
                f = lambda g: np.mean(np.power(chan, g)) - target                  # noqa: E731
                gamma = np.clip(found[0] if found else (0.1 if abs(f(0.1)) < abs(f(10)) else 10), 0.1, 10)
            assert np.array_equal(out, np.power(chan, gamma)), (kind, shape, target)
            gammas.append(float(gamma))
            arrays[R.key(kind, shape, "gamma_%g" % target)] = out.astype(np.float32)
        arrays[R.key(kind, shape, "gammas")] = np.asarray(gammas, dtype=np.float64)

    path = os.path.join(HERE, "photometric.npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s: %d arrays, %.1f KiB" % (path, len(arrays), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
