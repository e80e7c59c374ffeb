"""The first-order bounds of codebook_bound.py hold for an fp32 emulation of the codebook kernels' arithmetic in adversarial summation orders, and
they are tight enough to catch a kernel that rounds an operand to 11 bits or drops a member (no GPU)."""
import numpy as np
import pytest

import codebook_bound as B


def _orders(D, mags, rng):
    return {"ascending k": np.arange(D), "descending k": np.arange(D)[::-1], "largest terms first": np.argsort(-mags), "smallest terms first": np.argsort(mags),
            "random": rng.permutation(D)}


@pytest.mark.parametrize("F,K,D", [(37, 5, 8), (20, 30, 100), (9, 17, 512)])
def test_squared_distance_bound_holds_in_every_order(F, K, D):
    rng = np.random.default_rng(D)
    x = rng.normal(0, 1, (F, D)).astype(np.float32) * np.float32(10) ** rng.uniform(-2, 2, (F, 1)).astype(np.float32)
    c = (x[rng.integers(0, F, K)] + rng.normal(0, 0.05, (K, D))).astype(np.float32)          # near some features: cancellation in xx + cc - 2 x.c
    ref, bound = B.d2_ref(x, c)
    worst = 0.0
    for name, order in _orders(D, np.abs(x).mean(0) * np.abs(c).mean(0), rng).items():
        q = float((np.abs(B.d2_fp32(x, c, order).astype(np.float64) - np.maximum(ref, 0)) / bound).max())
        print("D = %d, %s: max |d2 - d2_64| / bound = %.3f" % (D, name, q))
        worst = max(worst, q)
    assert worst <= 1.0, worst
    # an operand rounded to fp16 (11 bits) is far outside (the worst-case bound grows with D, a random rounding error with its root: not at D = 512)
    q16 = float((np.abs(B.d2_fp32(x.astype(np.float16).astype(np.float32), c, np.arange(D)).astype(np.float64) - ref) / bound).max())
    assert q16 > 4.0 or D > 100, q16


@pytest.mark.parametrize("m,D", [(1, 16), (37, 16), (300, 8)])
def test_member_sum_bound_holds_in_every_order(m, D):
    rng = np.random.default_rng(m)
    terms = rng.normal(0, 1, (m, D)) * 10.0 ** rng.uniform(-3, 3, (m, 1))
    ref, bound = terms.sum(0), B.gamma(m) * np.abs(terms).sum(0)
    mags = np.abs(terms).sum(1)
    for name, order in {"member order": np.arange(m), "largest first": np.argsort(-mags), "smallest first": np.argsort(mags)}.items():
        q = B.within(B.sum_fp32(terms, order), ref, bound)
        print("m = %d, %s: max |S - S_64| / bound = %.3f" % (m, name, q))
        assert q <= 1.0, (name, q)
    if m > 1:                                                            # a dropped member is outside
        assert B.within(B.sum_fp32(terms, np.arange(m - 1)), ref, bound) > 1.0


def test_descriptor_bounds_cover_fp32_evaluation():
    rng = np.random.default_rng(5)
    S = rng.normal(0, 3, (2, 7, 16))
    S[0, 3] = 0.0                                                        # an untouched centroid
    E = 1e-6 * np.abs(S)
    S32 = (S + rng.uniform(-1, 1, S.shape) * E).astype(np.float32)       # sums anywhere inside their bound
    for name, param in (("l2norm", 0.0), ("normsign", 0.0), ("sigmoid", 3.0)):
        ref, bound = B.descriptor_ref(name, param, S, E)
        if name == "l2norm":
            got = S32 / (np.sqrt((S32 * S32).sum(-1, keepdims=True, dtype=np.float32)) + np.float32(1e-6))
        elif name == "normsign":
            got = np.sign(S32) / np.float32(np.sqrt(16.0))
        else:
            got = np.float32(2) * (np.float32(1) / (np.float32(1) + np.exp(-(np.float32(param) * S32)))) - np.float32(1)
        assert got.dtype == np.float32
        q = B.within(got, ref, bound)
        print("%s: max |d| / bound = %.3f" % (name, q))
        assert q <= 1.0, (name, q)
        assert (ref[0, 3] == 0).all()


def test_feature_functions_match_torch_formulas():
    import torch
    from gandtr_amd.components.model.layers.grouping import Grouping
    rng = np.random.default_rng(6)
    x, c, a = rng.normal(0, 1, (11, 16)), rng.normal(0, 1, (11, 16)), rng.uniform(0.5, 2, 11)
    for name in B.FEATURES:
        ref = Grouping.feature_functions[name](torch.from_numpy(x), torch.from_numpy(a).unsqueeze(1), torch.from_numpy(c)).numpy()
        assert np.abs(B.feature_values(name, x, a, c) - ref).max() <= 1e-12, name


def test_codebook_arguments_are_checked_before_any_launch():
    """the C entry points refuse bad sizes and null buffers on the host (ValueError), so this runs without a GPU"""
    import ctypes
    from gandtr_amd import _hip
    lib = _hip.load()
    need = ctypes.c_size_t()
    _hip.check(lib.gdt_codebook_nearest_workspace_bytes(131072, 65536, 128, 3, 0, ctypes.byref(need)))
    assert need.value >= (131072 + 65536) * 4 + 2 * 131072 * 3 * 4
    for args in ((0, 5, 8, 1, 0), (4, 0, 8, 1, 0), (4, 5, 0, 1, 0), (4, 5, 8193, 1, 0), (4, 5, 8, 0, 0), (4, 5, 8, 9, 0), (4, 5, 8, 1, 1025)):
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_codebook_nearest_workspace_bytes(*args, ctypes.byref(need)))
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_codebook_nearest(None, None, None, None, 4, 5, 8, 1, 0, None, 0, None))
    _hip.check(lib.gdt_codebook_aggregate_workspace_bytes(57, 7, 3, 3, ctypes.byref(need)))
    for args in ((57, 0, 3, 3), (57, 7, 9, 3), (57, 7, 3, 0), (1 << 29, 7, 8, 1), (57, 1 << 30, 3, 4)):
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_codebook_aggregate_workspace_bytes(*args, ctypes.byref(need)))
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_codebook_aggregate(None, None, None, None, None, None, None, None, 57, 7, 16, 3, 3, 0, 0, 0.0, None, 0, None))
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_kmeans_update(None, None, None, None, 300, 7, 8, None, 0, None))
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_local_descriptors_workspace_bytes(1, 2, 2, 48, 0, ctypes.byref(need)))
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_local_descriptors(None, 0, 1, 2, 2, 64, 1e-6, 0, None, None, None, 0, None))
