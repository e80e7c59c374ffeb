"""csrc/codebook.hip on the device: gdt_codebook_nearest, gdt_codebook_aggregate and gdt_kmeans_update against float64 under the derived bounds
of codebook_bound.py, and their bit-level guarantees (slices, repeated runs, ties, NaN rows, images on their own)."""
import numpy as np
import pytest
import torch

import codebook_bound as B

pytestmark = pytest.mark.gpu

NEAREST_CASES = [(37, 5, 8, 1), (300, 70, 100, 3), (129, 1000, 512, 5), (64, 4100, 24, 8), (5, 3, 16, 8)]
SIZES = (37, 0, 20)


def _data(F, K, D, seed=0):
    rng = np.random.default_rng(1000 * seed + F + K + D)
    x = rng.normal(0, 1, (F, D)).astype(np.float32)
    c = rng.normal(0, 1, (K, D)).astype(np.float32)
    c[: min(K, F) // 2] = x[: min(K, F) // 2] + rng.normal(0, 0.05, (min(K, F) // 2, D)).astype(np.float32)      # some centroids close to features
    return x, c


def _nearest(dev, x, c, ma, slices=0):
    from gandtr_amd import codebook
    d, i = codebook.nearest(torch.from_numpy(x).to(dev), torch.from_numpy(c).to(dev), ma, slices)
    return i.cpu().numpy(), d.cpu().numpy()


@pytest.mark.parametrize("F,K,D,ma", NEAREST_CASES)
def test_nearest_against_float64_and_bitwise_over_slices(cuda_device, F, K, D, ma):
    x, c = _data(F, K, D)
    ids, dists = _nearest(cuda_device, x, c, ma)
    q = B.check_nearest(x, c, ids, dists, ma)
    print("nearest (%d, %d, %d, %d): max |d2 - d2_64| / bound = %.3f" % (F, K, D, ma, q))
    for slices in (0, 1, 2, 7):                                        # 0 again: two runs give the same bits
        i2, d2 = _nearest(cuda_device, x, c, ma, slices)
        assert np.array_equal(i2, ids) and np.array_equal(d2.view(np.int32), dists.view(np.int32)), slices


@pytest.mark.parametrize("F,K,D,ma", [(300, 1000, 100, 3), (64, 300, 24, 1)])
def test_nearest_ties_take_the_lower_id_and_nan_rows_are_never_returned(cuda_device, F, K, D, ma):
    x, c = _data(F, K, D, seed=1)
    c[K - 100] = c[3]                                                  # identical rows, tiles (and slices) apart
    x[0] = c[3] + np.float32(1e-3)
    c[5, D // 2] = np.nan
    x[1] = np.where(np.isnan(c[5]), 0, c[5])                           # feature 1 would sit on the NaN centroid
    for slices in (0, 1, 7):
        ids, dists = _nearest(cuda_device, x, c, ma, slices)
        B.check_nearest(x, c, ids, dists, ma)
        assert ids[0, 0] == 3, ids[0]
        if ma > 1:
            assert ids[0, 1] == K - 100 and dists[0, 0] == dists[0, 1], (ids[0], dists[0])
        assert not (ids == 5).any()


def test_nearest_middle_feature_tile(cuda_device):
    """19200 features against one centroid tile: left to the library this is the 64-feature tile (the 128-feature one leaves CUs idle, the 32-feature one
    is not needed), the one shape the cases above do not reach; a forced slice count takes the 128-feature tile: the same bits"""
    x, c = _data(19200, 5, 8)
    ids, dists = _nearest(cuda_device, x, c, 3)
    B.check_nearest(x, c, ids, dists, 3)
    i2, d2 = _nearest(cuda_device, x, c, 3, 1)
    assert np.array_equal(i2, ids) and np.array_equal(d2.view(np.int32), dists.view(np.int32))


def test_nearest_refuses_bad_arguments(cuda_device):
    from gandtr_amd import codebook
    x, c = torch.zeros(4, 8, device=cuda_device), torch.zeros(3, 8, device=cuda_device)
    for kwargs in (dict(ma=0), dict(ma=9), dict(slices=1025), dict(slices=-1)):
        with pytest.raises(ValueError):
            codebook.nearest(x, c, **kwargs)


# ---- aggregation ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def agg_case(cuda_device):
    """37 + 0 + 20 features, K = 7 (+ 2 centroids far away that nothing touches), D = 16: the device's own top-3 ids and softmax weights"""
    from gandtr_amd import codebook
    rng = np.random.default_rng(7)
    F, D = sum(SIZES), 16
    x = rng.normal(0, 1, (F, D)).astype(np.float32)
    c = np.concatenate([rng.normal(0, 1, (7, D)), rng.normal(50, 1, (2, D))]).astype(np.float32)
    att = rng.uniform(0.2, 3, F).astype(np.float32)
    xd, cd, ad = (torch.from_numpy(t).to(cuda_device) for t in (x, c, att))
    dists, ids = codebook.nearest(xd, cd, 3)
    ass = torch.softmax(-2.0 * dists, dim=1)
    assert not bool((ids >= 7).any())
    return dict(x=x, c=c, att=att, xd=xd, cd=cd, ad=ad, ids=ids, ass=ass, ids_np=ids.cpu().numpy(), ass_np=ass.cpu().numpy())


def _check_aggregate(a, feature, descriptor, param, sizes=SIZES, sl=slice(None)):
    from gandtr_amd import codebook
    grouped, stats = codebook.aggregate(a["xd"][sl], a["ad"][sl], a["cd"], a["ids"][sl], a["ass"][sl], sizes, feature, descriptor, param)
    r = B.aggregate_ref(a["x"][sl], a["att"][sl], a["c"], a["ids_np"][sl], a["ass_np"][sl], sizes, feature)
    ref, bound = B.descriptor_ref(descriptor, param, r["S"], r["E"])
    q = B.within(grouped.cpu().numpy(), ref, bound)
    print("aggregate %s / %s: max |d| / bound = %.3f" % (feature, descriptor, q))
    assert q <= 1.0, (feature, descriptor, q)
    for name in codebook.STATS:
        qs = B.within(stats[name].cpu().numpy(), r[name], r[name + "_b"])
        assert qs <= 1.0, (feature, name, qs)
    untouched = r["count"] == 0
    assert untouched[:, 7:].all()
    if 0 in sizes:
        assert untouched[list(sizes).index(0)].all()
    for name in codebook.STATS:
        assert (stats[name].cpu().numpy()[untouched] == 0).all(), name
    assert (grouped.cpu().numpy()[untouched] == 0).all()
    return grouped, stats


@pytest.mark.parametrize("feature", B.FEATURES)
def test_aggregate_every_feature_function(agg_case, feature):
    _check_aggregate(agg_case, feature, "l2norm", 0.0)


@pytest.mark.parametrize("descriptor,param", [("l2norm", 0.0), ("normsign", 0.0), ("sigmoid", 3.0)])
def test_aggregate_every_descriptor_function(agg_case, descriptor, param):
    _check_aggregate(agg_case, "iden", descriptor, param)


def test_aggregate_bits_repeat_and_do_not_depend_on_the_other_images(agg_case):
    from gandtr_amd import codebook
    g1, s1 = _check_aggregate(agg_case, "normresatt", "l2norm", 0.0)
    g2, s2 = _check_aggregate(agg_case, "normresatt", "l2norm", 0.0)
    assert torch.equal(g1, g2) and all(torch.equal(s1[n], s2[n]) for n in codebook.STATS)
    start = 0
    for i, n in enumerate(SIZES):
        gi, si = _check_aggregate(agg_case, "normresatt", "l2norm", 0.0, sizes=(n,), sl=slice(start, start + n))
        assert torch.equal(gi[0], g1[i]) and all(torch.equal(si[name][0], s1[name][i]) for name in codebook.STATS), i
        start += n


@pytest.mark.parametrize("D", [130, 600, 2100])
def test_aggregate_wider_rows_take_the_other_workgroup_shapes(cuda_device, D):
    """D <= 128, <= 512, <= 2048 and beyond are four instantiations of the sum kernel"""
    from gandtr_amd import codebook
    rng = np.random.default_rng(D)
    x, c = rng.normal(0, 1, (40, D)).astype(np.float32), rng.normal(0, 1, (5, D)).astype(np.float32)
    att = rng.uniform(0.2, 3, 40).astype(np.float32)
    xd, cd, ad = (torch.from_numpy(t).to(cuda_device) for t in (x, c, att))
    dists, ids = codebook.nearest(xd, cd, 2)
    ass = torch.softmax(-0.1 * dists, dim=1)
    a = dict(x=x, c=c, att=att, xd=xd, cd=cd, ad=ad, ids=ids, ass=ass, ids_np=ids.cpu().numpy(), ass_np=ass.cpu().numpy())
    grouped, stats = codebook.aggregate(xd, ad, cd, ids, ass, (25, 15), "normresatt", "l2norm", 0.0)
    r = B.aggregate_ref(x, att, c, a["ids_np"], a["ass_np"], (25, 15), "normresatt")
    ref, bound = B.descriptor_ref("l2norm", 0.0, r["S"], r["E"])
    assert B.within(grouped.cpu().numpy(), ref, bound) <= 1.0
    assert B.within(stats["norm"].cpu().numpy(), r["norm"], r["norm_b"]) <= 1.0


def test_aggregate_many_rows_and_a_crowded_centroid(cuda_device):
    """3 x 750000 (image, centroid) rows: the exclusive scan of the member counts runs over more than 1024 blocks of 2048 (its carry loop), the members fill
    several count / place / rank blocks, and one centroid takes 1000 members (a long sum in member order); ids are given, not searched"""
    from gandtr_amd import codebook
    rng = np.random.default_rng(11)
    sizes, K, D, ma = (900, 0, 700), 750000, 2, 2
    F = sum(sizes)
    x = rng.normal(0, 1, (F, D)).astype(np.float32)
    c = rng.normal(0, 1, (K, D)).astype(np.float32)
    att = rng.uniform(0.2, 3, F).astype(np.float32)
    ids = rng.integers(0, K, (F, ma)).astype(np.int32)
    ids[:500, 0] = 123456
    ids[1000:1500, 1] = 123456
    ids[7, 1] = -1                                                        # a missing entry adds nothing
    ass = rng.uniform(0.1, 1, (F, ma)).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).to(cuda_device)
    grouped, stats = codebook.aggregate(dev(x), dev(att), dev(c), dev(ids), dev(ass), sizes, "resatt", "l2norm")
    r = B.aggregate_ref(x, att, c, ids, ass, sizes, "resatt")
    assert r["count"][0, 123456] == 500 and r["count"][2, 123456] == 500 and r["count"].sum() == F * ma - 1
    ref, bound = B.descriptor_ref("l2norm", 0.0, r["S"], r["E"])
    assert B.within(grouped.cpu().numpy(), ref, bound) <= 1.0
    for name in codebook.STATS:
        assert B.within(stats[name].cpu().numpy(), r[name], r[name + "_b"]) <= 1.0, name
    assert not grouped[1].any() and not stats["count"][1].any()


# ---- k-means -------------------------------------------------------------------------------------------------------------------------------

def test_kmeans_update_against_float64(cuda_device):
    from gandtr_amd import codebook
    pts, cen = B.blobs()
    gap, _ = B.assignment_gap(pts, cen, 1)
    d2, bound = B.d2_ref(pts, cen)
    assert (gap > 100 * bound.max(1)).all(), "precondition of the data: no assignment hangs on rounding"
    want = d2.argmin(1)
    p, c = torch.from_numpy(pts).to(cuda_device), torch.from_numpy(cen).to(cuda_device)
    _, ids = codebook.nearest(p, c, 1)
    assert np.array_equal(ids.cpu().numpy().reshape(-1), want)
    status = codebook.kmeans_update(p, ids, c)
    got = c.cpu().numpy()
    r = B.aggregate_ref(pts, None, cen, want.reshape(-1, 1).astype(np.int32), None, (300,), "iden")
    assert (r["count"][0, :6] == 50).all() and r["count"][0, 6] == 0
    ref, b = B.mean_ref(r["S"][0], r["E"][0], r["count"][0])
    q = B.within(got[:6], ref[:6], b[:6])
    print("k-means update: max |d| / bound = %.3f" % q)
    assert q <= 1.0, q
    assert np.array_equal(got[6].view(np.int32), cen[6].view(np.int32)), "a cluster without members keeps its centroid's bits"
    assert int(status.item()) & 1
    c2 = torch.from_numpy(cen[:6].copy()).to(cuda_device)
    assert int(codebook.kmeans_update(p, ids, c2).item()) == 0 and torch.equal(c2, c[:6])
