"""numpy restatements (float64, ``np.linalg.eigh``) of the three formulas behind the PCA whitening stages, and the seeded inputs of their tests:
    pcawhitenlearn                      mdir/external/cirtorch/utils/whiten.py:14-35
    paste_pca_normalize, l2_normalize   mdir/stages/whiten.py:99-135
The reference uses ``np.linalg.eig``; on these symmetric matrices ``eigh`` gives the same eigenpairs up to sign and rounding (tests/golden/
make_pca_whiten_golden.py prints how closely), in guaranteed real arithmetic."""
import numpy as np

PCA_CASES = [(16, 200, None), (32, 400, 8)]                      # (d, n, shrink) of the fixture
PASTE_CASES = [(16, 16, 300, 8), (32, 31, 500, 20), (64, 66, 900, None)]       # (d1, d2, n, dimensions) of the fixture
PASTE_STORED_ROWS = 4           # the last paste case stores every 4th output row (rows are independent without `dimensions`): file size


def descriptors(seed, d, n):
    """anisotropic unit-norm descriptor rows (the construction of tests/golden/make_whiten_golden.py: synth_set), N x D float32"""
    rng = np.random.default_rng(seed)
    basis = rng.normal(size=(d, d)) * (np.linspace(1.5, 0.2, d)[None, :])
    base = rng.normal(size=(n // 2, d)) @ basis.T
    X = np.concatenate([base, base + 0.3 * rng.normal(size=base.shape) @ basis.T])
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


def paste_inputs(case):
    d1, d2, n, _ = PASTE_CASES[case]
    return descriptors(100 + case, d1, n), descriptors(200 + case, d2, n)


def pcawhitenlearn(X, shrink=None):
    """X: D x N float64.  Returns (m, P, raw eigenvalues decreasing, eigenvalues after shrinkage)."""
    N = X.shape[1]
    m = X.mean(axis=1, keepdims=True)
    Xc = X - m
    Xcov = np.dot(Xc, Xc.T)
    Xcov = (Xcov + Xcov.T) / (2 * N)
    eigval, eigvec = np.linalg.eigh(Xcov)
    eigval, eigvec = eigval[::-1], eigvec[:, ::-1]
    shrunk = eigval
    if shrink:
        b = eigval[shrink - 1]
        shrunk = (1 - b) * eigval + b
    P = eigvec.T / np.sqrt(shrunk)[:, None]
    return m, P, eigval, shrunk


def paste_pca_normalize(data, dimensions=None):
    value = np.concatenate([np.asarray(x, dtype=np.float64) for x in data], axis=1)
    if dimensions:
        value = value - np.mean(value)
        _, eigvec = np.linalg.eigh(value.T.dot(value))
        vecs = eigvec[:, -dimensions:]
        value = value.dot(vecs.dot(vecs.T))
    return value / np.linalg.norm(value, axis=1, keepdims=True)


def l2_normalize(values):
    values = np.asarray(values, dtype=np.float64)
    return values / np.linalg.norm(values, axis=1, keepdims=True)


def rows_up_to_sign_abs(P, Q):
    """max over rows of min(|P_i - Q_i|_2, |P_i + Q_i|_2): absolute, for unit rows"""
    return float(np.minimum(np.linalg.norm(P - Q, axis=1), np.linalg.norm(P + Q, axis=1)).max())
