"""numpy float64 restatement of the diffusion on the mutual kNN graph (gandtr_amd/csrc/retrieval_diffusion.hip).  Row conventions
of the C ABI: ids / scores [n][k], seed_ids / seed_w [nq][kq], score matrices [n][nq].  Nothing here is rounded to fp32."""
import numpy as np


def affinity(scores, ids, gamma):
    """-> (w [n][k] mutual weights, S [n][k] normalised weights, deg [n]) in float64"""
    scores, ids = np.asarray(scores, dtype=np.float64), np.asarray(ids)
    n, k = ids.shape
    a = np.power(np.maximum(scores, 0.0), float(gamma))
    w = np.zeros((n, k))
    for i in range(n):
        for s in range(k):
            j = int(ids[i, s])
            if j < 0 or j >= n:
                continue
            t = np.nonzero(ids[j] == i)[0]
            if t.size:
                w[i, s] = min(a[i, s], a[j, t[0]])
    deg = np.zeros(n)
    for s in range(k):                                                  # s ascending
        deg = deg + w[:, s]
    r = np.where(deg == 0, 1.0, 1.0 / np.sqrt(np.where(deg == 0, 1.0, deg)))
    valid = (ids >= 0) & (ids < n)
    S = np.where(valid, w * (r[:, None] * r[np.where(valid, ids, 0)]), 0.0)
    return w, S, deg


def dense(S, ids):
    """the [n][k] weights as an n x n matrix (repeated ids of a row add, as the device's sum over the slots does)"""
    n, k = ids.shape
    valid = (ids >= 0) & (ids < n)
    rows = np.repeat(np.arange(n), k).reshape(n, k)
    out = np.zeros((n, n))
    np.add.at(out, (rows[valid], ids[valid]), np.asarray(S, dtype=np.float64)[valid])
    return out


def seeds(seed_ids, seed_w, n):
    """y [n][nq]: y[seed_ids[q][t], q] += seed_w[q][t]"""
    seed_ids, seed_w = np.asarray(seed_ids), np.asarray(seed_w, dtype=np.float64)
    nq, kq = seed_ids.shape
    valid = (seed_ids >= 0) & (seed_ids < n)
    cols = np.repeat(np.arange(nq), kq).reshape(nq, kq)
    y = np.zeros((n, nq))
    np.add.at(y, (seed_ids[valid], cols[valid]), seed_w[valid])
    return y


def solve(Sd, y, alpha):
    return np.linalg.solve(np.eye(Sd.shape[0]) - alpha * Sd, y)


def true_residual(Sd, y, f, alpha):
    """||y - (I - alpha S) f|| / ||y|| per column (0 where y = 0)"""
    f = np.asarray(f, dtype=np.float64)
    num = np.linalg.norm(y - (f - alpha * (Sd @ f)), axis=0)
    den = np.linalg.norm(y, axis=0)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def cg(Sd, y, alpha, tol, max_iter):
    """conjugate gradients from f = 0 with the device's stopping rule -> (f [n][nq], iterations [nq], relative recurrence residual [nq])"""
    n, nq = y.shape
    x, r, p = np.zeros((n, nq)), y.copy(), y.copy()
    rr = np.einsum("ij,ij->j", r, r)
    yy = rr.copy()
    its = np.zeros(nq, dtype=np.int32)
    live = (yy > 0) & (np.sqrt(rr) > tol * np.sqrt(yy))
    while live.any():
        c = np.nonzero(live)[0]                                         # the columns still running: the others are frozen
        ap = p[:, c] - alpha * (Sd @ p[:, c])
        a = rr[c] / np.einsum("ij,ij->j", p[:, c], ap)
        x[:, c] += a * p[:, c]
        r[:, c] -= a * ap
        rr_new = np.einsum("ij,ij->j", r[:, c], r[:, c])
        p[:, c] = r[:, c] + (rr_new / rr[c]) * p[:, c]
        rr[c] = rr_new
        its[c] += 1
        live[c] = (its[c] < max_iter) & (np.sqrt(rr[c]) > tol * np.sqrt(yy[c]))
    return x, its, np.where(yy > 0, np.sqrt(rr) / np.sqrt(np.where(yy > 0, yy, 1.0)), 0.0)


def knn(vecs, k):
    """float64 kNN lists of the rows of vecs other than themselves, strict order (score descending, id ascending); the tail is id -1 / -inf"""
    v = np.asarray(vecs, dtype=np.float64)
    n = v.shape[0]
    s = v @ v.T
    np.fill_diagonal(s, -np.inf)
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    sc = np.take_along_axis(s, order, axis=1)
    ids = np.where(np.isneginf(sc), -1, order).astype(np.int32)
    if k > n:
        ids = np.concatenate([ids, np.full((n, k - n), -1, np.int32)], axis=1)
        sc = np.concatenate([sc, np.full((n, k - n), -np.inf)], axis=1)
    return sc, ids


def strict_ranks(scores):
    """[n][nq] scores -> [n][nq] int32 database indices per column: score descending, id ascending (-0.0 == 0.0)"""
    s = np.asarray(scores, dtype=np.float64) + 0.0
    return np.argsort(-s, axis=0, kind="stable").astype(np.int32)


def clustered(seed, n, d, clusters, noise):
    """n unit rows around `clusters` random unit centres"""
    rng = np.random.RandomState(seed)
    c = rng.randn(clusters, d)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    g = rng.randn(n, d)
    v = c[rng.randint(0, clusters, n)] + noise * g / np.linalg.norm(g, axis=1, keepdims=True)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def arcs(seed, classes, per, degrees, d, noise):
    """`classes` arc manifolds: `per` points spread evenly over a great-circle arc of `degrees` in a random plane of R^d, plus `noise` times a normal
    vector, renormalised.  -> (unit rows [classes * per][d] fp32, labels)"""
    rng = np.random.RandomState(seed)
    out = []
    t = np.deg2rad(np.linspace(0.0, degrees, per))
    for _ in range(classes):
        q, _r = np.linalg.qr(rng.randn(d, 2))
        out.append(np.cos(t)[:, None] * q[:, 0] + np.sin(t)[:, None] * q[:, 1] + noise * rng.randn(per, d))
    v = np.concatenate(out)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32), np.repeat(np.arange(classes), per)


def arc_ground_truth(labels, per):
    """queries = the first point of every arc: positives the rest of its arc, the query itself junk"""
    gnd = []
    for c in range(len(labels) // per):
        q = c * per
        gnd.append({"ok": np.nonzero(labels == c)[0][1:], "junk": np.array([q])})
    return gnd


def self_seeds(scores, ids, cols, kq, gamma):
    """database-side seeds of the columns `cols`: the column itself with weight 1, then the first kq entries of its kNN row"""
    cols = np.asarray(cols)
    sid = np.concatenate([cols[:, None], np.asarray(ids)[cols, :kq]], axis=1).astype(np.int32)
    sw = np.concatenate([np.ones((len(cols), 1)), np.power(np.maximum(np.asarray(scores, dtype=np.float64)[cols, :kq], 0.0), float(gamma))], axis=1)
    return sid, sw
