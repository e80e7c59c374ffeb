"""Codebooks on the device (gandtr_amd/csrc/codebook.hip): nearest centroids of local descriptors without the features x centroids distance
matrix, their aggregation per image over the centroids, and the k-means update.  Inference only: inputs are detached.  The layers that use it:
``components/model/layers/grouping.py`` and ``functional.iterate_kmeans``."""
import ctypes

import torch

from . import _hip

FEATURE_FUNCTIONS = ("iden", "att", "res", "resatt", "normres", "normresatt", "normresatt2")
DESCRIPTOR_FUNCTIONS = ("l2norm", "normsign", "sigmoid")
STATS = ("count", "max_ass", "sum_ass", "max_assatt", "sum_assatt", "sum_assatt2", "norm")
MAX_MA = 8


def _rows(name, t):
    if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 2):
        raise ValueError("%s: a 2-D tensor on a HIP device is needed" % name)
    return t.detach().float().contiguous()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def nearest(x, c, ma=1, slices=0):
    """x [F][D], c [K][D] -> (dists fp32 [F][ma], ids int32 [F][ma]): per feature the ``ma`` nearest centroids in the strict order (squared
    distance ascending, id ascending); id -1 / distance +inf past the codebook's size.  slices = 0: the library's choice (same bits for any)."""
    x, c = _rows("x", x), _rows("c", c)
    if x.device != c.device or x.shape[1] != c.shape[1]:
        raise ValueError("features and centroids must share the device and the dimension")
    lib = _hip.load()
    (F, D), K = x.shape, c.shape[0]
    need = ctypes.c_size_t()
    _hip.check(lib.gdt_codebook_nearest_workspace_bytes(F, K, D, int(ma), int(slices), ctypes.byref(need)))
    with torch.cuda.device(x.device):
        ws = torch.empty(need.value, dtype=torch.uint8, device=x.device)
        dists = torch.empty((F, int(ma)), dtype=torch.float32, device=x.device)
        ids = torch.empty((F, int(ma)), dtype=torch.int32, device=x.device)
        _hip.check(lib.gdt_codebook_nearest(x.data_ptr(), c.data_ptr(), ids.data_ptr(), dists.data_ptr(), F, K, D, int(ma), int(slices),
                                            ws.data_ptr(), ws.numel(), _stream(x.device)))
    return dists, ids


def aggregate(x, att, c, ids, assign, image_sizes, feature="iden", descriptor="l2norm", descriptor_param=0.0):
    """x [F][D], att [F] or None, c [K][D], ids int32 [F][ma], assign fp32 [F][ma] or None, image_sizes: features per image (they are grouped
    by image, an image may be empty) -> (grouped fp32 [I][K][D], stats: dict of fp32 [I][K], keys ``STATS``)."""
    c = _rows("c", c)
    dev, (K, D), I = c.device, c.shape, len(image_sizes)
    F = int(sum(image_sizes))
    if ids.dim() != 2 or ids.shape[0] != F or ids.dtype != torch.int32 or min(image_sizes, default=0) < 0:
        raise ValueError("ids must be int32 [sum(image_sizes)][ma]")
    ma = ids.shape[1]
    lib = _hip.load()
    with torch.cuda.device(dev):
        grouped = torch.empty((I, K, D), dtype=torch.float32, device=dev)
        stats = torch.empty((len(STATS), I, K), dtype=torch.float32, device=dev)
        if I == 0:
            return grouped, dict(zip(STATS, stats))
        x = _rows("x", x) if F else None
        offsets = torch.tensor([0] + list(image_sizes), dtype=torch.int64).cumsum(0).to(dev)
        ids = ids.contiguous()
        att = att.detach().float().reshape(-1).contiguous() if att is not None else None
        assign = assign.detach().float().contiguous() if assign is not None else None
        if (att is not None and att.numel() != F) or (assign is not None and tuple(assign.shape) != (F, ma)) or (F and tuple(x.shape) != (F, D)):
            raise ValueError("x [F][D], att [F] and assign [F][ma] must match ids")
        need = ctypes.c_size_t()
        _hip.check(lib.gdt_codebook_aggregate_workspace_bytes(F, K, ma, I, ctypes.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        _hip.check(lib.gdt_codebook_aggregate(ptr(x), ptr(att), c.data_ptr(), ptr(ids), ptr(assign), offsets.data_ptr(), grouped.data_ptr(),
                                              stats.data_ptr(), F, K, D, ma, I, FEATURE_FUNCTIONS.index(feature),
                                              DESCRIPTOR_FUNCTIONS.index(descriptor), float(descriptor_param), ws.data_ptr(), ws.numel(), _stream(dev)))
    return grouped, dict(zip(STATS, stats))


def kmeans_update(x, ids, c):
    """c[k] <- mean of the points x[f] with ids[f] == k, in place (c: contiguous fp32 [K][D] on the device); returns the device status word (int32
    [1]): bit 0 is set when a cluster had no member and kept its centroid."""
    x = _rows("x", x)
    if not (c.is_cuda and c.dtype == torch.float32 and c.is_contiguous() and c.dim() == 2 and c.shape[1] == x.shape[1]):
        raise ValueError("c must be a contiguous fp32 [K][D] tensor on the device")
    ids = ids.reshape(-1).contiguous()
    if ids.dtype != torch.int32 or ids.numel() != x.shape[0]:
        raise ValueError("ids must be int32 [F]")
    lib = _hip.load()
    (F, D), K = x.shape, c.shape[0]
    need = ctypes.c_size_t()
    _hip.check(lib.gdt_kmeans_update_workspace_bytes(F, K, ctypes.byref(need)))
    with torch.cuda.device(x.device):
        ws = torch.empty(need.value, dtype=torch.uint8, device=x.device)
        status = torch.zeros(1, dtype=torch.int32, device=x.device)
        _hip.check(lib.gdt_kmeans_update(x.data_ptr(), ids.data_ptr(), c.data_ptr(), status.data_ptr(), F, K, D, ws.data_ptr(), ws.numel(),
                                         _stream(x.device)))
    return status
