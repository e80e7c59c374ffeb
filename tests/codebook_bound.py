"""Shared by test_codebook_bound_cpu.py, test_hip_codebook.py and test_hip_grouping.py: float64 references of the codebook kernels
(csrc/codebook.hip) with a first-order bound per output element, and fp32 emulations in adversarial summation orders (no test in here).

u = 2^-24 is the fp32 unit round-off: every fp32 operation returns its exact result times (1 + d), |d| <= u.

SQUARED DISTANCE.  d2 = max(0, fmaf(-2, x.c, xx + cc)).  x.c is D exact products added by D fp32 additions in some order: an error of at most
D u sum_k |x_k c_k| <= D u |x| |c| whatever the order (first order).  xx and cc are sums of D rounded squares, at most D roundings on any path of
any summation tree: D u xx and D u cc.  The addition xx + cc and the fmaf add one rounding each, u (xx + cc) + u d2 <= 2 u (|x| + |c|)^2.  Together
    |d2 - d2_64| <= D u (xx + cc + 2 |x| |c|) + 2 u (|x| + |c|)^2 = (D + 2) u (|x| + |c|)^2 <= (D + 4) u (|x| + |c|)^2,
the bound the tests use (the clamp at 0 only moves a value towards the non-negative truth).  The kernel returns sqrtf(d2), correctly rounded:
squaring the returned distance in float64 brings d2 back within 2 u d2, which the comparison adds.

MEMBER SUM.  S = sum over m members of t_e = assign_e * feature_e, each added by one fmaf in a fixed order: m roundings on the path, so
|S - S_64| <= m u sum |t_e| to first order, plus the rounding of the elementwise feature function itself, k_f u sum |t_e| with k_f roundings
relative to the feature value (``feature_roundings``: a product by the attention 1, a difference 1, the L2 normalisation the (D + 5) / 2 of its
sum of squares under the square root, whose own terms carry the difference's rounding twice, and 3 for sqrtf, + 1e-6 and the division).
"""
import numpy as np

U = 2.0 ** -24
FEATURES = ("iden", "att", "res", "resatt", "normres", "normresatt", "normresatt2")
DESCRIPTORS = ("l2norm", "normsign", "sigmoid")
EPS = float(np.float32(1e-6))


def gamma(k):
    return k * U / (1 - k * U)


# ---- nearest -------------------------------------------------------------------------------------------------------------------------------

def d2_ref(x, c):
    """float64 squared distances [F][K] of the stored fp32 rows, and the bound per entry"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    d2 = ((x[:, None, :] - c[None, :, :]) ** 2).sum(-1) if x.shape[0] * c.shape[0] * x.shape[1] <= 1 << 24 else \
        np.maximum((x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2 * x @ c.T, 0)
    nx, nc = np.sqrt((x * x).sum(1)), np.sqrt((c * c).sum(1))
    return d2, d2_bound(x.shape[1], nx[:, None], nc[None, :])


def d2_bound(D, norm_x, norm_c):
    return (D + 4) * U * (norm_x + norm_c) ** 2


def d2_fp32(x, c, order):
    """an fp32 emulation of the kernel's arithmetic with the three sums taken in the order ``order`` (a permutation of range(D)): sequential fp32
    additions of exact products (x.c) and of rounded squares (xx, cc)"""
    x, c = np.asarray(x, np.float32), np.asarray(c, np.float32)
    dot = np.zeros((x.shape[0], c.shape[0]), np.float32)
    xx, cc = np.zeros(x.shape[0], np.float32), np.zeros(c.shape[0], np.float32)
    for k in order:
        dot = (dot.astype(np.float64) + x[:, k].astype(np.float64)[:, None] * c[:, k].astype(np.float64)[None, :]).astype(np.float32)   # fmaf: one rounding
        xx = (xx.astype(np.float64) + x[:, k].astype(np.float64) ** 2).astype(np.float32)
        cc = (cc.astype(np.float64) + c[:, k].astype(np.float64) ** 2).astype(np.float32)
    t = (xx[:, None] + cc[None, :]).astype(np.float32)
    v = (t.astype(np.float64) - 2.0 * dot.astype(np.float64)).astype(np.float32)
    return np.maximum(v, np.float32(0))


def check_nearest(x, c, ids, dists, ma):
    """every assertion the issue lists for one nearest result (numpy arrays); returns the largest |d2 - d2_64| / bound seen"""
    F, K = x.shape[0], c.shape[0]
    d2, bound = d2_ref(x, c)
    ok = ~np.isnan(d2)                                               # a centroid row with a NaN has NaN distances: never returned
    valid = min(ma, int(ok[0].sum()))
    assert ids.shape == (F, ma) and dists.shape == (F, ma)
    assert (ids[:, valid:] == -1).all() and np.isposinf(dists[:, valid:]).all(), "tail must be id -1, distance +inf"
    got = ids[:, :valid].astype(np.int64)
    assert (got >= 0).all() and (got < K).all()
    rows = np.arange(F)[:, None]
    assert ok[rows, got].all(), "a NaN centroid was returned"
    assert all(len(set(r)) == valid for r in got), "a centroid was returned twice"
    dd = dists[:, :valid].astype(np.float64)
    assert (np.diff(dd, axis=1) >= 0).all(), "distances must ascend"
    ref, b = d2[rows, got], bound[rows, got]
    err = np.abs(dd ** 2 - ref) / (b + 2 * U * ref)
    assert err.max() <= 1.0, ("squared distance outside the bound", err.max())
    # validity: no centroid left out is closer than a returned one by more than the two bounds
    lo = np.where(ok, d2 + bound, np.inf)
    lo[rows, got] = np.inf
    assert ((ref - b) <= lo.min(1, keepdims=True)).all(), "a returned centroid is beaten by one left out"
    # ties in the device's own d2 are ordered by id
    tie = np.diff(dists[:, :valid], axis=1) == 0
    assert (np.diff(got, axis=1)[tie] > 0).all(), "equal distances must come in ascending id"
    return float(err.max())


def assignment_gap(x, c, ma):
    """per feature: (d2 of the (ma+1)-th nearest - d2 of the ma-th) in float64, and the ma-th squared distance"""
    d2 = np.sort(d2_ref(x, c)[0], axis=1)
    return d2[:, ma] - d2[:, ma - 1], d2[:, ma - 1]


# ---- aggregation ---------------------------------------------------------------------------------------------------------------------------

def feature_roundings(name, D):
    """k_f: roundings of the feature function relative to its value"""
    norm = 2 + (D + 5) / 2 + 3
    return {"iden": 0, "att": 1, "res": 1, "resatt": 2, "normres": norm, "normresatt": norm + 1, "normresatt2": norm + 2}[name]


def feature_values(name, x, att, c):
    """float64 feature function on member rows: x [M][D], att [M], c [M][D]"""
    a = att[:, None]
    r = x - c
    n = r / (np.sqrt((r * r).sum(1, keepdims=True)) + EPS)
    return {"iden": x, "att": a * x, "res": r, "resatt": a * r, "normres": n, "normresatt": a * n, "normresatt2": a * a * n}[name]


def aggregate_ref(x, att, c, ids, assign, sizes, feature, assign_rel=None):
    """float64 replay of gdt_codebook_aggregate's sums on the device's own ids / assign: dict with S [I][K][D] (the un-normalised sums), E (their
    bounds), the statistics [I][K] and their bounds ('<name>_b').  assign_rel [F][ma]: a relative error of the assignment weights themselves
    (grouping_ref: weights computed from rounded distances), carried into every bound; None when ``assign`` is the kernel's own input."""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    F, D = x.shape if x.size else (0, c.shape[1])
    K, I, ma = c.shape[0], len(sizes), ids.shape[1]
    att = np.ones(F) if att is None else np.asarray(att, np.float64).reshape(-1)
    assign = np.ones((F, ma)) if assign is None else np.asarray(assign, np.float64)
    img = np.repeat(np.arange(I), sizes)
    f, s = np.nonzero((ids >= 0) & (ids < K))
    k, w, a = ids[f, s].astype(np.int64), assign[f, s], att[f]
    rel = np.zeros(len(f)) if assign_rel is None else np.asarray(assign_rel, np.float64)[f, s]
    t = w[:, None] * feature_values(feature, x[f], a, c[k])
    key = (img[f], k)
    out = {n: np.zeros((I, K)) for n in ("count", "sum_ass", "sum_assatt", "sum_assatt2", "max_ass", "max_assatt", "abs_ass", "abs_assatt", "abs_assatt2")}
    S, T, R = np.zeros((I, K, D)), np.zeros((I, K, D)), np.zeros((I, K, D))
    np.add.at(S, key, t)
    np.add.at(T, key, np.abs(t))
    np.add.at(R, key, rel[:, None] * np.abs(t))
    out.update({n: np.zeros((I, K)) for n in ("rel_ass", "rel_assatt", "rel_assatt2", "rel_max")})
    np.add.at(out["count"], key, 1)
    for name, v in (("ass", w), ("assatt", w * a), ("assatt2", w * a * a)):
        np.add.at(out["sum_" + name], key, v)
        np.add.at(out["abs_" + name], key, np.abs(v))
        np.add.at(out["rel_" + name], key, rel * np.abs(v))
    np.maximum.at(out["rel_max"], key, rel * np.abs(w) * np.maximum(np.abs(a), 1))
    np.maximum.at(out["max_ass"], key, w)
    np.maximum.at(out["max_assatt"], key, w * a)
    m = out["count"]
    out["S"], out["E"] = S, gamma(m + feature_roundings(feature, D))[:, :, None] * T + R
    out["count_b"], out["max_ass_b"] = np.zeros((I, K)), out["rel_max"]
    out["max_assatt_b"] = U * np.abs(out["max_assatt"]) + out["rel_max"]
    out["sum_ass_b"] = gamma(m) * out["abs_ass"] + out["rel_ass"]
    out["sum_assatt_b"] = gamma(m + 1) * out["abs_assatt"] + out["rel_assatt"]
    out["sum_assatt2_b"] = gamma(m + 2) * out["abs_assatt2"] + out["rel_assatt2"]
    out["norm"] = np.sqrt((S * S).sum(-1))
    out["norm_b"] = norm_bound(S, out["E"])
    return out


def norm_bound(S, E):
    """|fp32 norm of the fp32 sums - ||S||: the sums' own error (||E||_2) plus the (D + 5) / 2 + 2 roundings of sum of squares, sqrtf"""
    D = S.shape[-1]
    return np.sqrt((E * E).sum(-1)) + gamma((D + 5) / 2 + 2) * np.sqrt((S * S).sum(-1))


def descriptor_ref(name, param, S, E):
    """float64 descriptor function of the sums and the bound per element.
    l2norm: o = S / (||S|| + 1e-6): E / den for the numerator, |o| times the denominator's relative error (norm_bound / den + u for the addition),
            + u for the division.
    normsign: sign(S) / sqrt(D) has no error but the division's u where the sign is decided (|S| > E); elsewhere any of the three signs is possible.
    sigmoid: o = 2 sigmoid(b S) - 1, |do/dS| = 2 |b| sigmoid (1 - sigmoid) <= |b| / 2: (|b| / 2) (E + u |S|) for the argument (its error and the
            product's rounding), 8 u for expf (2 ulp of a value whose effect on o is at most half of it), 1 + e, the reciprocal, 2 * and - 1 on values <= 2."""
    D = S.shape[-1]
    if name == "l2norm":
        den = np.sqrt((S * S).sum(-1, keepdims=True)) + EPS
        o = S / den
        return o, E / den + np.abs(o) * (norm_bound(S, E)[..., None] / den + 3 * U) + 1e-45
    if name == "normsign":
        o = np.sign(S) / np.sqrt(D)
        return o, np.where(np.abs(S) > E, 2 * U * np.abs(o), 1 / np.sqrt(D) + np.abs(o))
    o = 2 / (1 + np.exp(-param * S)) - 1
    return o, abs(param) / 2 * (E + U * np.abs(S)) + 8 * U


def mean_ref(S, E, count):
    """the k-means update: S / n, the sum's bound over n plus the division's rounding"""
    n = np.maximum(count, 1)[..., None]
    return S / n, E / n + U * np.abs(S / n)


def grouping_ref(x, att, c, sizes, feature, ma, assignment, base, descriptor, param, weights):
    """The hard-assignment grouping of one configuration in float64 from the stored fp32 inputs, with the bound an fp32 evaluation stays inside:
    dict grouped / grouped_b [I][K][D], weights / weights_b [I][K], ids [F][ma] (the float64 nearest centroids in the strict order).
    On top of the sum's own bound an fp32 evaluation computes the assignment weights from ROUNDED distances: a distance carries
    dd = min(d2_bound / (2 d), sqrt(d2_bound)) + u d (the square root of a squared distance inside d2_bound), a squared distance d2_bound + 3 u d2; a
    logit -b d (or -b d^2) then moves by |b| dd + u |logit|, a softmax weight by at most twice the largest move of a logit, relatively, plus
    (ma + 6) u for expf, the ma additions and the division.  Uniform weights are exact."""
    x64, c64 = np.asarray(x, np.float64), np.asarray(c, np.float64)
    F = x64.shape[0]
    d2, b2 = d2_ref(x, c)
    ids = np.argsort(d2, axis=1, kind="stable")[:, :ma].astype(np.int32)
    rows = np.arange(F)[:, None]
    dsel, bsel = d2[rows, ids], b2[rows, ids]
    if assignment == "uniform":
        w, rel = np.ones((F, ma)), np.zeros((F, ma))
    else:
        dist = np.sqrt(dsel)
        if assignment == "softmax":
            logit, dl = -base * dist, abs(base) * (np.minimum(bsel / np.maximum(2 * dist, 1e-300), np.sqrt(bsel)) + U * dist)
        else:
            logit, dl = -base * dsel, abs(base) * (bsel + 3 * U * dsel)
        dl = dl + U * np.abs(logit)
        e = np.exp(logit - logit.max(1, keepdims=True))
        w = e / e.sum(1, keepdims=True)
        rel = np.broadcast_to(2 * dl.max(1, keepdims=True) + (ma + 6) * U, (F, ma))
    r = aggregate_ref(x, att, c, ids, w, sizes, feature, assign_rel=rel)
    grouped, grouped_b = descriptor_ref(descriptor, param, r["S"], r["E"])
    n = np.maximum(np.asarray(sizes, np.float64), 1)[:, None]
    if weights == "unif":
        wv, wb = (r["count"] > 0).astype(np.float64), np.zeros_like(r["count"])
    elif weights in ("maxass", "maxassatt"):
        wv, wb = r["max_" + weights[3:]], r["max_" + weights[3:] + "_b"]
    elif weights in ("avgass", "avgassatt", "avgassatt2"):
        wv = r["sum_" + weights[3:]] / n
        wb = r["sum_" + weights[3:] + "_b"] / n + U * np.abs(wv)
    else:                                                            # descnorm3: the cube's derivative 3 norm^2, and two products
        wv = r["norm"] ** 3
        wb = 3 * (r["norm"] + r["norm_b"]) ** 2 * r["norm_b"] + 3 * U * wv
    return dict(grouped=grouped, grouped_b=grouped_b, weights=wv, weights_b=wb, ids=ids, sums=r)


def blobs(seed=3):
    """300 points in 6 blobs, D = 8, the blob centres (perturbed) and a seventh centroid far away"""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 10, (6, 8))
    pts = (centres[np.arange(300) % 6] + rng.normal(0, 1, (300, 8))).astype(np.float32)
    cen = np.concatenate([centres + rng.normal(0, 0.3, (6, 8)), np.full((1, 8), 300.0)]).astype(np.float32)
    return pts, cen


def sum_fp32(terms, order):
    """sequential fp32 sum of float64 terms [m][D] in the given member order, each term rounded to fp32 first (the product's rounding)"""
    acc = np.zeros(terms.shape[1], np.float32)
    for e in order:
        acc = (acc.astype(np.float64) + np.float32(terms[e]).astype(np.float64)).astype(np.float32)
    return acc


def within(got, ref, bound):
    """max |got - ref| / bound over the elements (0 where they agree exactly, inf where got is not finite)"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return float("inf")
    d = np.abs(got - ref)
    return float(np.where(d == 0, 0.0, d / np.maximum(bound, 1e-300)).max()) if d.size else 0.0
