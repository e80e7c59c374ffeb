"""Learned whitening ("Lw") on the device: produces the ``{"m", "P"}`` that ``cirwhiten`` applies.

Reference (numpy float64 on the CPU): ``whitenlearn(X, qidxs, pidxs)`` (mdir/external/cirtorch/utils/whiten.py:37-70), called by
the ``learn_lw_whitening`` stage with ``values.astype(float64).T`` and the index lists of matching (query, positive) pairs
(mdir/stages/whiten.py:30-75).  Same conventions here: ``X`` is D x N (one descriptor per column), the result is ``(m, P)`` with
``m`` D x 1 and ``P`` D x D float64.  The rows of ``P`` are eigenvectors times ``inv(cholesky(S))`` and therefore defined up to sign
(whitened descriptors differ by a per-dimension sign, scores between them do not).  No CPU fallback."""
import ctypes

import numpy as np
import torch

from . import _hip


def whitenlearn(X, qidxs, pidxs, return_info=False):
    """X: D x N tensor on a HIP device (any float dtype; the kernels read float32 rows and compute in float64);
    qidxs / pidxs: equally long sequences (or tensors) of column numbers.  Returns (m [D x 1], P [D x D]) float64 device tensors."""
    lib = _hip.load()
    if not isinstance(X, torch.Tensor) or not X.is_cuda or X.dim() != 2:
        raise ValueError("whitenlearn needs a D x N tensor on a HIP device")
    dev = X.device
    rows = X.t().contiguous().float()                                   # [N][D]
    n_vec, d = rows.shape
    q = torch.as_tensor(qidxs, dtype=torch.int64).reshape(-1)
    p = torch.as_tensor(pidxs, dtype=torch.int64).reshape(-1)
    if q.numel() != p.numel() or q.numel() == 0:
        raise ValueError("query and positive index lists must be non-empty and equally long")
    if int(q.min()) < 0 or int(p.min()) < 0 or int(q.max()) >= n_vec or int(p.max()) >= n_vec:
        raise IndexError("pair index out of range for %d vectors" % n_vec)
    q32, p32 = q.to(dev, torch.int32), p.to(dev, torch.int32)
    m = torch.empty((d,), dtype=torch.float64, device=dev)
    P = torch.empty((d, d), dtype=torch.float64, device=dev)
    eig = torch.empty((d,), dtype=torch.float64, device=dev)
    info = (ctypes.c_int * 2)()
    need = ctypes.c_size_t()
    with torch.cuda.device(dev):
        _hip.check(lib.gdt_whiten_learn_workspace_bytes(n_vec, d, q32.numel(), ctypes.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        _hip.check(lib.gdt_whiten_learn(rows.data_ptr(), q32.data_ptr(), p32.data_ptr(), n_vec, d, q32.numel(), m.data_ptr(),
                                        P.data_ptr(), eig.data_ptr(), info, ws.data_ptr(), ws.numel(),
                                        torch.cuda.current_stream(dev).cuda_stream))
    if return_info:
        return m[:, None], P, {"eigenvalues": eig, "cholesky_jitter_steps": info[0], "jacobi_sweeps": abs(info[1]),
                               "one_sided": info[1] > 0}        # False: the scatter matrix was singular, two-sided fallback
    return m[:, None], P


def learn_lw_whitening(names, values, queries, positives):
    """Host-side mirror of the ``learn_lw_whitening`` stage body (mdir/stages/whiten.py:30-75): names -> row numbers, then
    ``whitenlearn``.  ``values``: N x D tensor on the device.  Returns {"m": D x 1, "P": D x D} as float64 numpy arrays, the format
    ``CirtorchWhiten`` loads (wrapper.py:315-317)."""
    assert len(names) == len(values)
    assert len(queries) == len(positives)
    index = {x: i for i, x in enumerate(names)}
    q = [index[x] for x in queries]
    p = [index[x] for x in positives]
    m, P = whitenlearn(values.t(), q, p)
    return {"m": m.cpu().numpy(), "P": P.cpu().numpy()}


def pcawhitenlearn(X, shrink=None, return_info=False):
    """``pcawhitenlearn(X, shrink)`` (mdir/external/cirtorch/utils/whiten.py:14-35) on the device.  X: D x N tensor on a HIP device (the
    kernels read float32 rows and compute in float64, as ``whitenlearn`` above); ``shrink``: None / 0 for none, else 1..D (Arun's
    shrinkage, whiten.py:28-31).  Returns (m [D x 1], P [D x D]) float64 device tensors, ``P[i] = eigvec_i^T / sqrt(eigval'_i)`` with the
    eigenvalues decreasing; rows are defined up to sign.  D must be even (ValueError otherwise).

    A covariance that is numerically not positive definite -- some (shrunk) eigenvalue not above ``D * 2^-52`` times the largest, e.g.
    N <= D without ``shrink`` -- raises ``np.linalg.LinAlgError`` naming the eigenvalue.  The reference divides by the square root of
    whatever ``np.linalg.eig`` returned there and silently hands back infinite or NaN rows; that is not mirrored."""
    if not isinstance(X, torch.Tensor) or not X.is_cuda or X.dim() != 2:
        raise ValueError("pcawhitenlearn needs a D x N tensor on a HIP device")
    d, n_vec = X.shape
    shrink = int(shrink) if shrink else 0
    if d < 2 or d % 2 or d > 8192:
        raise ValueError("pcawhitenlearn: descriptor size must be even and <= 8192, got %d" % d)
    if n_vec < 1:
        raise ValueError("pcawhitenlearn: no vectors")
    if not 0 <= shrink <= d:
        raise ValueError("pcawhitenlearn: shrink must be in 1..%d, got %d" % (d, shrink))
    lib = _hip.load()
    dev = X.device
    rows = X.t().contiguous().float()                                   # [N][D]
    m = torch.empty((d,), dtype=torch.float64, device=dev)
    P = torch.empty((d, d), dtype=torch.float64, device=dev)
    eig = torch.empty((d,), dtype=torch.float64, device=dev)
    info = (ctypes.c_int * 1)()
    need = ctypes.c_size_t()
    with torch.cuda.device(dev):
        _hip.check(lib.gdt_pca_whiten_learn_workspace_bytes(n_vec, d, ctypes.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        rc = lib.gdt_pca_whiten_learn(rows.data_ptr(), n_vec, d, shrink, m.data_ptr(), P.data_ptr(), eig.data_ptr(), info, ws.data_ptr(),
                                      ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    if rc == _hip.GDT_ERR_INVALID:                  # (the arguments were checked above: what is left is the positive-definiteness test)
        raise np.linalg.LinAlgError(lib.gdt_last_error().decode("utf8", "replace"))
    _hip.check(rc)
    if return_info:
        return m[:, None], P, {"eigenvalues": eig, "jacobi_sweeps": abs(info[0]), "one_sided": info[0] > 0}
    return m[:, None], P


def pca_project_normalize(values, dimensions, return_info=False):
    """The ``dimensions`` branch of ``paste_pca_normalize`` (mdir/stages/whiten.py:108-125) on the device: ``values`` N x D (any width, odd
    included) on a HIP device, computed in float64.  Subtracts the scalar mean of the whole matrix, projects onto the span of the
    ``dimensions`` leading eigenvectors of ``values^T values`` (the result stays N x D) and divides every row by its norm, no epsilon."""
    if not isinstance(values, torch.Tensor) or not values.is_cuda or values.dim() != 2:
        raise ValueError("pca_project_normalize needs an N x D tensor on a HIP device")
    n, d = values.shape
    dimensions = int(dimensions)
    if n < 1 or not 1 <= d <= 8191:
        raise ValueError("pca_project_normalize: needs at least one row and a width of 1..8191, got %d x %d" % (n, d))
    if not 1 <= dimensions <= d:
        raise ValueError("pca_project_normalize: dimensions must be in 1..%d, got %d" % (d, dimensions))
    lib = _hip.load()
    dev = values.device
    v = values.to(torch.float64).contiguous()
    out = torch.empty_like(v)
    info = (ctypes.c_int * 1)()
    need = ctypes.c_size_t()
    with torch.cuda.device(dev):
        _hip.check(lib.gdt_pca_project_normalize_workspace_bytes(n, d, ctypes.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        _hip.check(lib.gdt_pca_project_normalize(v.data_ptr(), n, d, dimensions, out.data_ptr(), info, ws.data_ptr(), ws.numel(),
                                                 torch.cuda.current_stream(dev).cuda_stream))
    if return_info:
        return out, {"jacobi_sweeps": abs(info[0]), "one_sided": info[0] > 0}
    return out


def l2n_rows(values):
    """``values / np.linalg.norm(values, axis=1, keepdims=True)`` in float64 on the device, no epsilon (mdir/stages/whiten.py:125, :135)."""
    if not isinstance(values, torch.Tensor) or not values.is_cuda or values.dim() != 2:
        raise ValueError("l2n_rows needs an N x D tensor on a HIP device")
    lib = _hip.load()
    v = values.to(torch.float64).contiguous()
    out = torch.empty_like(v)
    if v.numel():
        with torch.cuda.device(v.device):
            _hip.check(lib.gdt_l2n_rows_f64(v.data_ptr(), out.data_ptr(), v.shape[0], v.shape[1], torch.cuda.current_stream(v.device).cuda_stream))
    return out
