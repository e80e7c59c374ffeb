"""Shared by tests/golden/make_photometric_golden.py and the photometric tests: the seeded input planes, the list of recorded cases, a float64
evaluation of the Lab formulas with the first-order error bound of the device's float32 chain, and the bound of its gamma output.  No test here."""
import numpy as np

SHAPES = [(1, 1), (33, 47), (64, 64), (100, 130)]
KINDS = ["smooth", "narrow", "constant", "black", "white", "two", "edges"]
NAMES = ["f3d_lab", "b166b47", "2cd274e"]
GAMMA_TARGETS = [0.05, 0.3, 0.5, 0.9, 0.999, 1e-6]
OTHER_SHAPE = (40, 50)                   # the second plane of channel2channel_histogram_matching: a size of its own


def edge_values():
    """the 256 centres, the 255 inner float32 edges (k + 0.5) / 255 and both float32 neighbours of each edge: 1021 values"""
    centres = np.linspace(0, 1, 256).astype(np.float32)
    edges = ((np.arange(255, dtype=np.float64) + 0.5) / 255).astype(np.float32)
    return np.concatenate([centres, edges, np.nextafter(edges, np.float32(-1)), np.nextafter(edges, np.float32(2))]).astype(np.float32)


def plane(kind, h, w, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * h + w)
    if kind == "smooth":                                   # smooth ramp + noise
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        base = 0.5 + 0.38 * np.sin(xx / max(w, 2) * 5 + seed) * np.cos(yy / max(h, 2) * 3)
        return np.clip(base + rng.normal(0, 0.03, (h, w)), 0, 1).astype(np.float32)
    if kind == "narrow":                                   # low contrast: most bins empty
        return np.clip(rng.normal(0.47, 0.02, (h, w)), 0, 1).astype(np.float32)
    if kind == "constant":
        return np.full((h, w), 0.25, np.float32)
    if kind == "black":
        return np.zeros((h, w), np.float32)
    if kind == "white":
        return np.ones((h, w), np.float32)
    if kind == "two":
        return np.where(rng.random((h, w)) < 0.3, np.float32(0.2), np.float32(0.7)).astype(np.float32)
    if kind == "edges":
        return np.resize(edge_values(), (h, w)).astype(np.float32)
    raise KeyError(kind)


def other_plane(seed=0):
    return plane("smooth", OTHER_SHAPE[0], OTHER_SHAPE[1], seed + 100)


def cases():
    """(kind, (h, w), [histograms], channel-to-channel?, [gamma targets]) of every recorded combination.  The two small shapes carry everything; the two
    large ones what keeps the file small: the noisy kinds, two targets, one or two gammas."""
    out = []
    for kind in KINDS:
        for shape in SHAPES[:2]:
            out.append((kind, shape, ["eq"] + NAMES, True, GAMMA_TARGETS))
    for kind in ("smooth", "narrow"):
        out.append((kind, SHAPES[2], ["eq", "f3d_lab"], True, [0.3]))
    out.append(("smooth", SHAPES[3], ["eq", "b166b47"], True, [0.5]))
    return out


def key(kind, shape, what):
    return "%s_%dx%d_%s" % (kind, shape[0], shape[1], what)


# ---- float64 Lab and the first-order bound of the device's float32 evaluation ----

_RGB2XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], np.float64)
_WHITE = np.array([0.950456, 1.0, 1.088754], np.float64)
U = 2.0 ** -24                           # unit roundoff of float32: one correctly rounded operation is within U relative, a 1-ulp function within 2 U


def lab_f64(rgb, in_scale=1.0, in_shift=0.0):
    """(normalised Lab [..., 3] in float64, per-component first-order error bound of the device chain) for rgb [..., 3] (any float dtype).

    The matrix is the device's: float32(rgb2xyz / white).  The bound follows the device's steps (gandtr_amd/csrc/lab_device.h), every term an absolute error:
      input affine   c = x * scale + shift: two roundings                                   -> 2 U |c|
      sRGB curve     lin = exp2(2.4 * log2(t)), t = (c + 0.055) * (1 / 1.055): the argument carries 3 roundings (sum, constant, product) and the affine's error,
                     amplified by 2.4 in relative terms; the exponent 2.4 * log2 t carries the constant's rounding, the product's and log2's 1 ulp (2 U), i.e. an
                     absolute error e = 4 U |2.4 log2 t|, which exp2 turns into the relative error e * ln 2; exp2's own 1 ulp (2 U).
                     Together  U (2 + 4 ln2 |2.4 log2 t|) + 2.4 (3 U + rel(c))  relative.
                     (linear branch: one rounding + the input's error)
      matrix row     v = m0 r + m1 g + m2 b: the inputs' errors weighted + 3 roundings of products and 2 of sums, all bounded by 5 U (|m0| r + |m1| g + |m2| b)
      cube root      f = exp2(log2(v) / 3): relative error  U (2 + 4 ln2 |log2(v) / 3|) + rel(v) / 3;  linear branch: 7.787 * err(v) + 2 U f
      L / 100        116 f - 16 (2 roundings of magnitudes <= 116 f), / 100 (1 rounding):  (116 err(f) + U (2 * 116 f + L)) / 100
      a, b           500 (fx - fy), 200 (fy - fz), + 128, / 255: (500 (err fx + err fy) + U (3 * 500 |fx - fy| + 2 * 128 + ...)) / 255, bounded below with 4 roundings
    """
    x = np.asarray(rgb, np.float64)
    c_raw = x * in_scale + in_shift
    err_c = 2 * U * np.abs(c_raw) + 0.0 * c_raw
    c = np.clip(c_raw, 0.0, 1.0)
    t = (c + 0.055) / 1.055
    hi = c > 0.04045
    lin = np.where(hi, t ** 2.4, c / 12.92)
    rel_t = 3 * U + err_c / np.maximum(c + 0.055, 1e-300)
    rel_lin = np.where(hi, U * (2 + 4 * np.log(2) * np.abs(2.4 * np.log2(t))) + 2.4 * rel_t, U + err_c / np.maximum(c, 1e-300))
    err_lin = np.where(c > 0, rel_lin * lin, err_c / 12.92)
    fwd = (_RGB2XYZ / _WHITE[:, None]).astype(np.float32).astype(np.float64)
    v = lin @ fwd.T
    err_v = err_lin @ np.abs(fwd).T + 5 * U * (np.abs(lin) @ np.abs(fwd).T)
    big = v > 0.008856
    vs = np.maximum(v, 1e-300)
    f = np.where(big, np.cbrt(vs), 7.787 * v + 16.0 / 116.0)
    err_f = np.where(big, f * (U * (2 + 4 * np.log(2) * np.abs(np.log2(vs) / 3)) + err_v / vs / 3), 7.787 * err_v + 2 * U * f)
    L = np.where(big[..., 1], 116.0 * f[..., 1] - 16.0, 903.3 * v[..., 1])
    err_L = np.where(big[..., 1], 116.0 * err_f[..., 1] + U * (2 * 116.0 * f[..., 1] + np.abs(L)), 903.3 * err_v[..., 1] + 2 * U * np.abs(L)) + U * np.abs(L)
    a = 500.0 * (f[..., 0] - f[..., 1])
    b = 200.0 * (f[..., 1] - f[..., 2])
    err_a = 500.0 * (err_f[..., 0] + err_f[..., 1]) + 4 * U * (np.abs(a) + 128.0)
    err_b = 200.0 * (err_f[..., 1] + err_f[..., 2]) + 4 * U * (np.abs(b) + 128.0)
    lab = np.stack([L / 100.0, (a + 128.0) / 255.0, (b + 128.0) / 255.0], axis=-1)
    bound = np.stack([err_L / 100.0, err_a / 255.0, err_b / 255.0], axis=-1)
    return lab, bound


def gamma_output_bound(x, gamma):
    """per-pixel bound of |device x^gamma - reference x^gamma| for float32 x in [0, 1]: the exponent may differ by 1e-4, the reference's own tolerance
    (first order: |x^g ln x| * 1e-4); the device evaluates pow in float64 and rounds to float32 once (U relative); the fixture holds the reference's value
    rounded to float32 once (U relative)."""
    x = np.asarray(x, np.float64)
    y = np.power(x, gamma)
    with np.errstate(divide="ignore", invalid="ignore"):
        sens = np.where(x > 0, np.abs(y * np.log(np.maximum(x, 1e-300))), 0.0)
    return sens * 1e-4 + 2 * U * np.abs(y) + 1e-45
