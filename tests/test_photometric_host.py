"""Host side of the photometric transforms (gandtr_amd/components/data/photometric.py) against tests/golden/photometric.npz, which
tests/golden/make_photometric_golden.py recorded from the reference's functional.py; class semantics on numpy pics; the registries; argument errors of the
C ABI.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from gandtr_amd import _hip, photometric
from gandtr_amd.components.data import photometric as P
from gandtr_amd.components.data import transform as T
from gandtr_amd.ingest import DeviceTransform
from oracle import clahe_oracle as C

import photometric_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photometric.npz")
MEAN_STD = ([0.5] * 3, [0.5] * 3)
NEW_NAMES = ["match_histogram", "replace_histogram", "gamma_equalize", "tospace", "add_intensity_fromrgb", "add_clahe_fromrgb"]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as data:
        arrays = {k: data[k] for k in data.files}
    assert sorted(photometric.load_histograms(GOLDEN)) == sorted(R.NAMES)
    return arrays


def test_named_histograms_come_from_the_fixture_only(golden):
    mode, cdf = photometric.target_cdf("f3d_lab")
    assert mode == photometric.MODE_TARGET and np.array_equal(cdf, np.cumsum(golden["histogram_f3d_lab"]))
    assert photometric.target_cdf("eq") == (photometric.MODE_EQ, None)
    with pytest.raises(KeyError):
        photometric.target_cdf("no_such_histogram")
    with pytest.raises(ValueError):
        photometric.register_histogram("short", np.ones(255))
    with pytest.raises(ValueError):
        photometric.register_histogram("eq", np.ones(256))


@pytest.mark.parametrize("case", R.cases(), ids=lambda c: "%s_%dx%d" % (c[0], c[1][0], c[1][1]))
def test_host_channel_functions_match_the_reference(golden, case):
    kind, shape, histograms, c2c, targets = case
    chan = R.plane(kind, *shape)
    for hist in histograms:
        got = P.channel_histogram_matching(chan.copy(), hist)
        assert got.dtype == np.float32 and np.array_equal(got, golden[R.key(kind, shape, "match_" + hist)]), hist
    if c2c:
        assert np.array_equal(P.channel2channel_histogram_matching(chan.copy(), R.other_plane()), golden[R.key(kind, shape, "c2c")])
    explicit = P.channel_histogram_matching(chan.copy(), golden["histogram_f3d_lab"])                  # 256 bin masses instead of a name
    assert np.array_equal(explicit, P.channel_histogram_matching(chan.copy(), "f3d_lab"))
    gammas = golden[R.key(kind, shape, "gammas")]
    for target, ref_gamma in zip(targets, gammas):
        gamma = float(P.gamma_of(chan, target))
        if ref_gamma in (0.1, 10.0):
            assert gamma == ref_gamma, (target, gamma)                                                 # clipped: exactly the bound
        else:
            assert abs(gamma - ref_gamma) <= 1e-4, (target, gamma, ref_gamma)                         # the reference's own tol
        out = P.channel_gamma_matching(chan, target)
        ref = golden[R.key(kind, shape, "gamma_%g" % target)]
        assert np.isfinite(out).all()
        assert (np.abs(out - ref.astype(np.float64)) <= R.gamma_output_bound(chan, ref_gamma)).all(), target
        if kind in ("black", "white"):
            assert np.array_equal(out, chan)


def test_clipped_targets_give_the_bounds_exactly(golden):
    chan = R.plane("smooth", 33, 47)
    assert float(P.gamma_of(chan, 0.999)) == 0.1 and float(P.gamma_of(chan, 1e-6)) == 10.0
    gammas = golden[R.key("smooth", (33, 47), "gammas")]
    assert gammas[4] == 0.1 and gammas[5] == 10.0


def test_secant_raises_where_newton_does():
    with pytest.raises(RuntimeError):
        P.secant(lambda g: 1.0, 0.5)                                      # equal function values at different points
    with pytest.raises(RuntimeError):
        P.secant(lambda g: float("nan"), 0.5)                             # never converges
    assert abs(P.secant(lambda g: g * g - 2.0, 1.0) - 2.0 ** 0.5) < 1e-6


def _rgb(seed, h, w, dark=False):
    rng = np.random.default_rng(seed)
    img = rng.random((h, w, 3)).astype(np.float32)
    return (img * np.float32(0.03)).astype(np.float32) if dark else img


@pytest.mark.parametrize("dark", [False, True])
def test_host_lab_against_the_oracle(dark):
    """Both sides evaluate the same float32 formulas with numpy.  Forward: each is within the first-order bound B of photometric_ref.lab_f64 of the float64
    value (numpy's pow and cbrt are within 1 ulp, like the device's exp2 / log2 the bound was written for), so they differ by at most 2 B.  Backward: about
    12 float32 roundings of magnitudes <= 5.2 (the largest absolute row sum of the inverse matrix) in front of the transfer curve, whose slope is at most
    12.92: 12 * 5.2 * 12.92 * 2^-24 = 4.8e-5."""
    img = _rgb(3, 37, 41, dark)
    got, ref = P.rgb2normspace(img), C.rgb2normspace_lab(img)
    assert got.dtype == np.float32 and got.shape == img.shape
    _, bound = R.lab_f64(img)
    assert (np.abs(got.astype(np.float64) - ref) <= 2 * bound).all()
    lab64, _ = R.lab_f64(img)
    assert (np.abs(got - lab64) <= bound).all()
    back, back_ref = P.normspace2rgb(got), C.normspace2rgb_lab(got)
    assert float(np.abs(back - back_ref).max()) <= 4.8e-5
    assert float(np.abs(back - img).max()) < 2e-3                          # and the pair is a round trip
    with pytest.raises(NotImplementedError):
        P.rgb2normspace(img, "luv")


def test_image_functions_compose_the_channel_functions(golden):
    img = _rgb(5, 33, 47)
    spc = C.rgb2normspace_lab(img)
    for hist in ("eq", "f3d_lab"):
        ref = spc.copy()
        ref[:, :, 0] = P.channel_histogram_matching(spc[:, :, 0], hist)
        assert float(np.abs(P.image_histogram_matching(img, hist) - C.normspace2rgb_lab(ref)).max()) <= 4.8e-5
    ref = spc.copy()
    ref[:, :, 0] = P.channel_gamma_matching(spc[:, :, 0], 0.3)
    assert abs(float(ref[:, :, 0].mean()) - 0.3) < 1e-4                        # the lightness mean moved to the target
    assert float(np.abs(P.image_gamma_matching(img, 0.3) - C.normspace2rgb_lab(ref)).max()) <= 4.8e-5


def test_class_semantics_on_numpy_pics(golden):
    rgb = _rgb(7, 33, 47)
    four = np.concatenate([rgb, R.plane("smooth", 33, 47)[:, :, None]], axis=2)
    other = np.concatenate([_rgb(8, 40, 50), R.other_plane()[:, :, None]], axis=2)
    # replace_histogram, constant histogram: append / replace
    out = P.ReplaceChannelWithHistogram("f3d_lab", "append")(four)
    assert isinstance(out, tuple) and len(out) == 1 and out[0].shape == (33, 47, 5)
    assert np.array_equal(out[0][:, :, 4], golden[R.key("smooth", (33, 47), "match_f3d_lab")]) and np.array_equal(out[0][:, :, :4], four)
    out = P.ReplaceChannelWithHistogram("eq", "replace")(four, other)[0]
    assert out.shape == (33, 47, 4) and np.array_equal(out[:, :, :3], rgb)
    # ... with a second pic: matched to its last channel, which is stripped
    out0, out1 = P.ReplaceChannelWithHistogram("eq", "replace")(four, other)
    assert np.array_equal(out0[:, :, 3], golden[R.key("smooth", (33, 47), "c2c")]) and out1.shape == (40, 50, 3)
    out0, out1 = P.ReplaceChannelWithHistogram("eq", "append")(four, other)
    assert out0.shape == (33, 47, 5) and np.array_equal(out1, other[:, :, :3])
    with pytest.raises(AssertionError):
        P.ReplaceChannelWithHistogram("eq", "prepend")
    # the others
    assert P.ToColorspace("lab")(four)[0].shape == (33, 47, 3)
    added = P.AddIntensityFromRgb()(four)[0]
    assert added.shape == (33, 47, 5) and np.array_equal(added[:, :, 4], P.rgb2normspace(rgb)[:, :, 0])
    assert np.array_equal(P.MatchHistogram("eq")(rgb)[0], P.image_histogram_matching(rgb, "eq"))
    assert np.array_equal(P.GammaEqualize("0.3")(rgb)[0], P.image_gamma_matching(rgb, 0.3))
    for bad in ("0", "1", "1.5"):
        with pytest.raises(AssertionError):
            P.GammaEqualize(bad)
    for build in (lambda: P.MatchHistogram("eq", "luv"), lambda: P.GammaEqualize(0.3, "hsv"), lambda: P.ToColorspace("luv"),
                  lambda: P.AddIntensityFromRgb("yxz"), lambda: P.AddClaheFromRgb(4, 8, "luv")):
        with pytest.raises(NotImplementedError):
            build()


def test_repr_is_the_reference_form():
    assert repr(P.MatchHistogram("f3d_lab")) == "MatchHistogram(histogram=f3d_lab, colorspace=lab)"
    assert repr(P.ReplaceChannelWithHistogram("eq", "append")) == "ReplaceChannelWithHistogram(histogram=eq, created_channel=append)"
    assert repr(P.GammaEqualize("0.3")) == "GammaEqualize(target=0.3, colorspace=lab)"
    assert repr(P.ToColorspace("lab")) == "ToColorspace(colorspace=lab)"
    assert repr(P.AddIntensityFromRgb()) == "AddIntensityFromRgb(colorspace=lab)"
    assert repr(P.AddClaheFromRgb("2", "4")) == "AddClaheFromRgb(clip_limit=2.0, grid_size=4, colorspace=lab)"


def test_registries():
    assert sorted(P.TRANSFORMS) == sorted(NEW_NAMES) and not set(P.TRANSFORMS) & set(T.TRANSFORMS)
    chain = ("pil2np | tospace:lab | add_intensity_fromrgb | add_clahe_fromrgb:2:4 | match_histogram:eq:lab | gamma_equalize:0.3 | "
             "replace_histogram:eq:append | totensor | normalize")
    steps = P.initialize_transforms(chain, MEAN_STD).transforms
    assert [type(s).__name__ for s in steps] == ["Pil2Numpy", "ToColorspace", "AddIntensityFromRgb", "AddClaheFromRgb", "MatchHistogram", "GammaEqualize",
                                                 "ReplaceChannelWithHistogram", "ToTensor", "Normalize"]
    assert steps[5].params == {"target": 0.3, "colorspace": "lab"} and steps[3].params["grid_size"] == 4
    out = P.initialize_transforms("pil2np | match_histogram:eq | totensor | normalize", MEAN_STD)((_rgb(1, 16, 20) * 255).astype(np.uint8))
    assert isinstance(out, torch.Tensor) and out.shape == (3, 16, 20)
    for name in NEW_NAMES:                                               # the old registry and the default constructor do not know them
        with pytest.raises(KeyError):
            T.initialize_transforms("pil2np | %s | totensor" % name, MEAN_STD)
        with pytest.raises(KeyError):
            DeviceTransform("pil2np | %s | totensor" % name, MEAN_STD)


def test_device_transform_photometric_option():
    t = DeviceTransform("pil2np | centerscalecrop:32_32:0.8 | match_histogram:eq | totensor | normalize", MEAN_STD, photometric=True)
    assert t.photometric == ("match_histogram", "eq") and t.clahe_clip is None and [n for n, _ in t.geometric] == ["centerscalecrop"]
    t = DeviceTransform("pil2np | gamma_equalize:0.3:lab | totensor", MEAN_STD, photometric=True)
    assert t.photometric == ("gamma_equalize", 0.3) and t.geometric == []
    assert DeviceTransform("pil2np | totensor | normalize", MEAN_STD, photometric=True).photometric is None
    for chain in ("pil2np | match_histogram:eq | mirror | totensor",                           # before a geometric step
                  "pil2np | gamma_equalize:0.3 | center_crop:8_8 | totensor",
                  "pil2np | apply_clahe:1.0 | match_histogram:eq | totensor",                 # together with apply_clahe
                  "pil2np | gamma_equalize:0.3 | apply_clahe:1.0 | totensor",
                  "pil2np | match_histogram:eq | gamma_equalize:0.3 | totensor",              # two of them
                  "pil2np | match_histogram:eq:luv | totensor"):
        with pytest.raises(NotImplementedError):
            DeviceTransform(chain, MEAN_STD, photometric=True)
    with pytest.raises(AssertionError):
        DeviceTransform("pil2np | gamma_equalize:1.5 | totensor", MEAN_STD, photometric=True)
    for name in ("tospace:lab", "replace_histogram:eq:append", "random_crop:224"):            # the option opens the two names only
        with pytest.raises(KeyError):
            DeviceTransform("pil2np | %s | totensor" % name, MEAN_STD, photometric=True)


def test_c_abi_argument_errors_without_gpu():
    lib = _hip.load()
    need = ctypes.c_size_t()
    _hip.check(lib.gdt_photometric_workspace_bytes(2, 33, 47, ctypes.byref(need)))
    assert need.value >= 2 * (2 * 256 * 4 + 256 * 8 + 33 * 47 * 4)
    one = ctypes.c_void_p(256)                                            # a non-null address that is never touched: every check comes first
    for call in (lambda: lib.gdt_photometric_workspace_bytes(0, 8, 8, ctypes.byref(need)),
                 lambda: lib.gdt_photometric_workspace_bytes(1, 0, 8, ctypes.byref(need)),
                 lambda: lib.gdt_photometric_workspace_bytes(1, 1 << 14, 1 << 14, ctypes.byref(need)),
                 lambda: lib.gdt_photometric_workspace_bytes(1, 8, 8, None),
                 lambda: lib.gdt_lab_lightness_f32(None, one, 1, 8, 8, None, None, None),
                 lambda: lib.gdt_rgb2lab_f32(one, None, 1, 8, 8, None, None, None),
                 lambda: lib.gdt_hist256_f32(one, 1, 0, one, one, None),
                 lambda: lib.gdt_hist256_f32(one, 1, 64, None, one, None),
                 lambda: lib.gdt_match_channel_f32(one, one, 1, 64, 7, None, None, 0, one, one, 1 << 20, None),        # unknown mode
                 lambda: lib.gdt_match_channel_f32(one, one, 1, 64, 1, None, None, 0, one, one, 1 << 20, None),        # target mode without a cdf
                 lambda: lib.gdt_match_channel_f32(one, one, 1, 64, 2, None, None, 0, one, one, 1 << 20, None),        # plane mode without a plane
                 lambda: lib.gdt_match_histogram_lab_f32(one, one, 1, 8, 8, None, None, None, None, 2, None, one, one, 1 << 20, None),
                 lambda: lib.gdt_match_histogram_lab_f32(one, one, 1, 8, 8, None, None, None, (ctypes.c_float * 3)(1, 0, 1), 0, None, one, one, 1 << 20, None),
                 lambda: lib.gdt_gamma_channel_f32(one, one, 1, 64, 1.0, one, None, None),
                 lambda: lib.gdt_gamma_channel_f32(one, one, 1, 64, 0.3, None, None, None),
                 lambda: lib.gdt_gamma_equalize_lab_f32(one, one, 1, 8, 8, None, None, None, None, 0.0, one, None, one, 1 << 20, None)):
        with pytest.raises(ValueError):
            _hip.check(call())
    with pytest.raises(RuntimeError):                                     # a workspace that is too small is its own status
        _hip.check(lib.gdt_match_channel_f32(one, one, 1, 64, 0, None, None, 0, one, one, 16, None))
    for fn in (photometric.lightness, photometric.to_lab, photometric.histogram256, lambda t: photometric.match_channel(t, "eq"),
               lambda t: photometric.match_histogram(t, "eq"), lambda t: photometric.gamma_channel(t, 0.3), lambda t: photometric.gamma_equalize(t, 0.3)):
        with pytest.raises(ValueError):
            fn(torch.zeros(1, 3, 8, 8))                                   # not on a device
