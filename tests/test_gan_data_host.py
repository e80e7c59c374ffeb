"""The GAN scenarios' data layer on the host (no GPU): DeviceTransform.plan and the host transforms against the reference's recorded crops, flips and
picks (tests/golden/gan_data.npz), the numpy bilinear step against tests/crop_resize_ref.py and against torch's bilinear interpolation, the datasets
and the loader on a CPU device, and the argument checks of the crop-resize C ABI."""
import ctypes
import os
import pickle
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crop_resize_ref as REF                                   # noqa: E402
import gan_data_fixture as FX                                   # noqa: E402

from gandtr_amd.components.data import transform as T           # noqa: E402
from gandtr_amd.ingest import DeviceTransform, Geometry         # noqa: E402

MEAN_STD = [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gan_data.npz"))


# ---- geometry against the reference's draws ----

@pytest.mark.parametrize("name", sorted(FX.CROP_CASES))
def test_plan_reproduces_the_reference_crops(golden, name):
    chain, shapes = FX.CROP_CASES[name]
    transform = DeviceTransform("pil2np | %s | totensor | normalize" % chain, MEAN_STD)
    for row, seed in enumerate(FX.SEEDS):
        random.seed(seed)
        if golden[name + "_refused"][row]:
            with pytest.raises(AssertionError):
                transform.plan(shapes)
            continue
        plan = transform.plan(shapes)
        assert random.random() == golden[name + "_next"][row], "the chain drew a different count of random numbers"
        for pic, g in enumerate(plan):
            assert isinstance(g, Geometry)
            assert list(g.box) == golden[name + "_box"][row, pic].tolist(), (seed, pic)
            assert int(g.flip_src) == golden[name + "_flip_src"][row, pic] and int(g.flip_dst) == golden[name + "_flip_dst"][row, pic], (seed, pic)
            assert int(g.resample[0] == "bilinear") == golden[name + "_resampled"][row, pic]


def test_plan_takes_any_rng():
    transform = DeviceTransform("scalecrop:16_16:0.8_1 | mirror", MEAN_STD)
    a = transform.plan([(37, 53)], random.Random(3))
    random.seed(3)
    assert a == transform.plan([(37, 53)])


@pytest.mark.parametrize("name", sorted(FX.CROP_CASES))
def test_host_transforms_reproduce_the_reference_crops(golden, name):
    """the host Compose on coordinate pics: the pixels it returns are those of the recorded box, mirrored as recorded.  Geometry only: a resized
    result is compared with ``bilinear_resize`` of the recorded box, the code under test, whose arithmetic the bilinear tests below check against
    tests/crop_resize_ref.py and torch"""
    chain, shapes = FX.CROP_CASES[name]
    compose = T.initialize_transforms(chain, MEAN_STD)
    for row, seed in enumerate(FX.SEEDS):
        pics = [FX.coordinate_pic(h, w) for h, w in shapes]
        random.seed(seed)
        if golden[name + "_refused"][row]:
            with pytest.raises(AssertionError):
                compose(*pics)
            continue
        out = compose(*pics)
        assert random.random() == golden[name + "_next"][row]
        out = [out] if len(shapes) == 1 else list(out)
        for pic, res in enumerate(out):
            y0, x0, ch, cw = golden[name + "_box"][row, pic]
            want = pics[pic][y0:y0 + ch, x0:x0 + cw]
            if golden[name + "_flip_src"][row, pic]:
                want = want[:, ::-1]
            if golden[name + "_resampled"][row, pic]:
                size = T.parse_tuple([s for s in chain.split("|") if "scalecrop" in s][0].split(":")[1])
                want = T.bilinear_resize(want, size[0], size[1])
            if golden[name + "_flip_dst"][row, pic]:
                want = want[:, ::-1]
            assert np.array_equal(res, want), (seed, pic)


@pytest.mark.parametrize("name", sorted(FX.DOWNSCALE_CASES))
def test_host_downscale_is_pillows(golden, name):
    (h, w), n = FX.DOWNSCALE_CASES[name]
    pic = FX.photo(11, h, w).astype(np.float32) / 255.0
    out = T.initialize_transforms("downscale:%d" % n, MEAN_STD)(pic)
    assert np.array_equal(out, golden[name])
    g, = DeviceTransform("pil2np | downscale:%d | totensor" % n, MEAN_STD).plan([(h, w)])
    assert g.out == golden[name].shape[:2] and g.resample == (("lanczos", n) if max(h, w) > n else ("none",))


# ---- the bilinear step ----

BILINEAR_SHAPES = [((37, 53), 16, 16), ((17, 16), 16, 16), ((300, 411), 256, 256), ((320, 320), 256, 256), ((257, 256), 256, 256), ((512, 700), 256, 256)]


@pytest.mark.parametrize("shape,ow,oh", BILINEAR_SHAPES + [((17, 20), 16, 16), ((23, 31), 18, 10), ((32, 32), 16, 16), ((16, 16), 16, 16)])
def test_host_bilinear_matches_the_float64_reference(shape, ow, oh):
    u8 = FX.photo(3, *shape)
    got = T.bilinear_resize(u8.astype(np.float32) / np.float32(255), ow, oh).transpose(2, 0, 1)
    ref = REF.crop_resize(u8, (0, 0, shape[0], shape[1]), ow, oh)
    assert got.dtype == np.float32 and got.shape == ref.shape
    err = np.abs(got.astype(np.float64) - ref)
    print("max |host - ref| = %.3e, gate at that element %.3e" % (err.max(), REF.gate(ref).flat[err.argmax()]))
    assert (err <= REF.gate(ref)).all()


@pytest.mark.parametrize("shape,ow,oh", BILINEAR_SHAPES)
def test_bilinear_formula_is_torchs_at_power_of_two_outputs(shape, ow, oh):
    """an independent implementation of the same coordinate map: F.interpolate(bilinear, align_corners=False) in float64"""
    u8 = FX.photo(4, *shape)
    unit = (u8.astype(np.float32) / np.float32(255)).astype(np.float64)
    ref = REF.resize_unit(unit, ow, oh)
    tor = torch.nn.functional.interpolate(torch.from_numpy(unit).permute(2, 0, 1)[None], size=(oh, ow), mode="bilinear", align_corners=False)[0]
    err = np.abs(tor.permute(1, 2, 0).numpy() - ref).max()
    print("max |torch f64 - ref| = %.3e" % err)
    assert err <= 2.0 ** -20


def test_identity_tables_when_the_box_has_the_output_size():
    for n in (1, 7, 16, 256):
        s0, s1, f = T.linear_taps(n, n)
        assert s0.tolist() == list(range(n)) and not f.any()


# ---- construction, repr, refusals ----

def test_initialize_transforms_builds_every_new_name():
    chain = "pil2np | mirror:0.25 | center_crop:40_30 | square_crop | downscale:24 | scalecrop:16_16:0.8_1 | centerscalecrop:8_8:0.9 | totensor | normalize"
    compose = T.initialize_transforms(chain, MEAN_STD)
    text = repr(compose)
    for part in ("RandomHorizontalFlip(p=0.25)", "CenterCrop(size=[30 40])", "SquareCrop()", "Downscale(size=24)", "RandomScaleCrop(size=[16 16], scale=(0.8, 1.0))",
                 "CenterScaleCrop(size=[8 8], scale=(0.9, 0.9))"):
        assert part in text, text
    out = compose(FX.photo(0, 50, 60))
    assert out.shape == (3, 8, 8) and out.dtype == torch.float32
    assert set(T.TRANSFORMS) >= {"mirror", "center_crop", "square_crop", "downscale", "scalecrop", "centerscalecrop"}
    assert T.RandomScaleCrop("16_16").params["scale"] == (0.5, 0.8) and T.CenterScaleCrop("16_16").params["scale"] == (0.6, 0.6)


def test_published_chains_run_on_the_host_without_cv2():
    random.seed(0)
    x, y = T.initialize_transforms("pil2np | scalecrop:256_256:0.8_1 | totensor | normalize", MEAN_STD)(FX.photo(0, 300, 411), FX.photo(1, 280, 500))
    assert x.shape == y.shape == (3, 256, 256) and float(x.min()) >= -1 and float(x.max()) <= 1
    out = T.initialize_transforms("pil2np | downscale:362 | totensor | normalize", MEAN_STD)(FX.photo(2, 400, 724))
    assert out.shape == (3, 200, 362)


@pytest.mark.parametrize("chain", ["scalecrop:16_16 | center_crop:8_8", "downscale:32 | scalecrop:16_16", "scalecrop:16_16 | downscale:8", "downscale:16 | square_crop",
                                   "apply_clahe:1.0 | scalecrop:16_16"])
def test_unsupported_chain_shapes_are_refused(chain):
    with pytest.raises(NotImplementedError, match="scalecrop|downscale"):
        DeviceTransform("pil2np | %s | totensor" % chain, MEAN_STD)


@pytest.mark.parametrize("name", ["random_crop:224", "gaussian_noise:0.1", "tospace:lab", "match_histogram", "gamma_equalize"])
def test_other_names_keep_raising_key_error(name):
    with pytest.raises(KeyError):
        DeviceTransform("pil2np | %s | totensor" % name, MEAN_STD)
    with pytest.raises(KeyError):
        T.initialize_transforms("pil2np | %s | totensor" % name, MEAN_STD)


def test_chains_without_geometry_keep_their_attributes():
    t = DeviceTransform("pil2np | apply_clahe:1.0 | totensor | normalize", MEAN_STD)
    assert (t.mean, t.std, t.clahe_clip, t.clahe_grid, t.normalize, t.geometric) == ([0.5] * 3, [0.5] * 3, 1.0, 8, True, [])
    assert t.plan([(5, 7)]) == [Geometry((0, 0, 5, 7), False, ("none",), False, (5, 7))]
    with pytest.raises(NotImplementedError):
        DeviceTransform("pil2np | mirror | totensor", MEAN_STD)(None)


# ---- datasets and the loader on a CPU device ----

@pytest.fixture()
def files(tmp_path):
    from PIL import Image
    sizes = {"X0": (40, 50), "X1": (33, 47), "X2": (40, 40), "Y0": (36, 36), "Y1": (50, 41)}
    for name, (h, w) in sizes.items():
        Image.fromarray(FX.photo(len(name) + h, h, w)).save(str(tmp_path / (name + ".jpg")), quality=90)
    (tmp_path / "day.txt").write_text("X0.jpg\nX1.jpg\nX2.jpg\n")
    (tmp_path / "night.txt").write_text("Y0.jpg\nY1.jpg\n")
    with open(str(tmp_path / "tuples.pkl"), "wb") as f:
        pickle.dump({"val": [["X0.jpg", "Y0.jpg"], ["X1.jpg", "Y1.jpg", "X2.jpg"]]}, f)
    return tmp_path


def _train(files, size=5, batch_size=2, chain="pil2np | scalecrop:16_16:0.8_1 | totensor | normalize"):
    return {"dataset": {"name": "RandomDomainsPair", "dataset_X": str(files / "day.txt"), "dataset_Y": str(files / "night.txt"), "image_dir": str(files) + "/*",
                        "size": size},
            "loader": {"batch_size": batch_size}, "transforms": chain, "mean_std": MEAN_STD}


def test_mdir_alias_resolves():
    import mdir                                                  # noqa: F401
    from mdir.components.data import dataset
    from gandtr_amd.components.data import dataset as own
    assert dataset is own
    assert set(dataset.DATASET_LABELS) == {"ImageList", "InferImageList", "RandomImageTuple", "PregeneratedImageTuple", "RandomDomainsPair"}


def test_domain_pairs_on_cpu(files, golden):
    from gandtr_amd.components.data import dataset as D
    loader = D.initialize_dataset_loader(None, "train", _train(files), device="cpu")
    assert len(loader.dataset) == 5 and len(loader) == 3
    np.random.seed(0)
    loader.dataset.prepare_epoch(None, None)
    random.seed(1)
    batches = list(loader)
    assert [b[0].shape for b in batches] == [(2, 3, 16, 16), (2, 3, 16, 16), (1, 3, 16, 16)]
    assert all(len(b) == 2 and b[1].shape == b[0].shape and b[0].dtype == torch.float32 for b in batches)
    for name, (nx, ny, size, seed) in FX.PAIR_CASES.items():
        ds = D.RandomDomainsPairDataset(None, None, str(files / "day.txt"), str(files / "night.txt"), str(files) + "/*", size)
        ds.images_X, ds.images_Y = ["x"] * nx, ["y"] * ny
        np.random.seed(seed)
        ds.prepare_epoch(None, None)
        assert [int(i) for i in ds.idxs_X] == golden[name + "_X"].tolist() and [int(i) for i in ds.idxs_Y] == golden[name + "_Y"].tolist()
        assert len(ds) == int(golden[name + "_len"])
    assert len(D.RandomDomainsPairDataset(None, None, str(files / "day.txt"), str(files / "night.txt"), str(files), None)) == 2


def test_mixed_sizes_raise_runtime_error_on_cpu(files):
    from gandtr_amd.components.data import dataset as D
    loader = D.initialize_dataset_loader(None, "train", _train(files, chain="pil2np | totensor | normalize"), device="cpu")
    loader.dataset.idxs_X, loader.dataset.idxs_Y = [0, 1, 0, 0, 0], [0, 0, 0, 0, 0]
    with pytest.raises(RuntimeError):
        next(iter(loader))


def test_pregenerated_tuples(files, golden, tmp_path):
    from gandtr_amd.components.data import dataset as D
    names = FX.tuple_names()
    with open(str(tmp_path / "golden_tuples.pkl"), "wb") as f:
        pickle.dump({"val": names}, f)
    for idx in FX.TUPLE_IDX:
        ds = D.PregeneratedImageTupleDataset(None, None, str(tmp_path / "golden_tuples.pkl"), "val", str(tmp_path) + "/*", idx)
        assert ds.epoch_idxs == golden["tuple_" + idx].tolist(), idx
        assert ds.files(1) == [str(tmp_path / names[1][i]) for i in ds.epoch_idxs[1]]
        assert ds.prepare_epoch(None, None) is None and ds.epoch_idxs == golden["tuple_" + idx].tolist()
    val = {"dataset": {"name": "PregeneratedImageTuple", "image_dir": str(files) + "/*", "dataset": str(files / "tuples.pkl"), "data_key": "val", "idx": "0_1"},
           "loader": {"batch_size": 1}, "transforms": "pil2np | totensor | normalize", "mean_std": MEAN_STD}
    loader = D.initialize_dataset_loader(None, "val", val, device="cpu")
    shapes = [[tuple(t.shape) for t in b] for b in loader]
    assert shapes == [[(1, 3, 40, 50), (1, 3, 36, 36)], [(1, 3, 33, 47), (1, 3, 50, 41)]]
    with pytest.raises(NotImplementedError):
        D.RandomImageTupleDataset(None, None, str(files / "tuples.h5"), "val", str(files), "0_1")


def test_random_tuple_get_idx():
    from gandtr_amd.components.data.dataset import RandomImageTupleDataset as R
    assert R.get_idx(-1, 5, [], None) == 4 and R.get_idx(2, 5, [], None) == 2
    assert R.get_idx("any", 5, [], lambda n: n - 1) == 4
    assert R.get_idx("different", 5, [0, 4], lambda n: n - 1) == 3
    assert R.get_idx((1, None), 5, [], lambda a, b: (a, b)) == (1, 5) and R.get_idx([None, -2], 5, [], lambda a, b: (a, b)) == (0, -2)
    with pytest.raises(AssertionError):
        R.get_idx(5, 5, [], None)


def test_infer_image_list_on_cpu(files):
    from gandtr_amd.components.data import dataset as D
    params = {"dataset": {"name": "InferImageList", "image_dir": str(files)}, "loader": {"batch_size": 2},
              "transforms": "pil2np | downscale:32 | totensor | normalize", "mean_std": MEAN_STD}
    loader = D.initialize_dataset_loader([["X2", "Y0", "X2"]], "test", params, device="cpu")
    assert len(loader) == 2
    (names, images), (names2, images2) = list(loader)
    assert names == [("X2", "Y0")] and names2 == [("X2",)]
    assert images.shape == (2, 3, 32, 32) and images2.shape == (1, 3, 32, 32) and torch.equal(images[0], images2[0])
    plain = D.initialize_dataset_loader([["X0", "X1"], ["Y0", "Y1"]], "train",
                                        {"dataset": {"name": "ImageList", "image_dir": str(files), "data_cols": "0:"}, "loader": {"batch_size": 1},
                                         "transforms": "pil2np | centerscalecrop:16_16:0.8 | totensor", "mean_std": MEAN_STD}, device="cpu")
    assert [[tuple(t.shape) for t in b] for b in plain] == [[(1, 3, 16, 16)] * 2] * 2


def test_loader_refusals(files):
    from gandtr_amd.components.data import dataset as D
    params = _train(files)
    params["sampler"] = {}
    with pytest.raises(AssertionError):
        D.initialize_dataset_loader(None, "train", params, device="cpu")
    for name in ("CirTuples", "CirDiverseAnchors", "CirImageList"):
        with pytest.raises(NotImplementedError, match="mining|validation"):
            D.initialize_dataset_loader(None, "train", {"dataset": {"name": name}, "loader": {"batch_size": 1}, "transforms": "pil2np | totensor",
                                                         "mean_std": MEAN_STD}, device="cpu")
    with pytest.raises(RuntimeError, match="Unsupported stage"):
        D.initialize_dataset(None, "infer", None, {"name": "ImageList"})
    shuffled = D.initialize_dataset_loader(None, "train", _train(files, size=4, batch_size=4), loader_default_params={"shuffle": True, "num_workers": 2}, device="cpu")
    assert shuffled.shuffle and len(shuffled) == 1


# ---- the C ABI's argument checks (before any HIP call) ----

def test_crop_resize_argument_errors():
    from gandtr_amd import _hip
    lib = _hip.load()
    need = ctypes.c_size_t()
    _hip.check(lib.gdt_crop_resize_workspace_bytes(3, 18, 10, ctypes.byref(need)))
    assert need.value >= 3 * (18 + 10) * 8
    for bad in ((0, 16, 16), (1, 0, 16), (1, 16, 0)):
        with pytest.raises(ValueError):
            _hip.check(lib.gdt_crop_resize_workspace_bytes(*bad, ctypes.byref(need)))
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_crop_resize_workspace_bytes(1, 16, 16, None))

    def call(n=1, ow=16, oh=16, src=0x1000, dst=0x2000, h=20, w=30, box=(2, 1, 17, 18), ws=0x3000, ws_bytes=None, std=None, items=True):
        arr = (_hip.CropItem * max(n, 1))()
        for it in arr:
            it.src, it.h, it.w, it.dst_chw = src, h, w, dst
            it.x0, it.y0, it.cw, it.ch = box
        size = ctypes.c_size_t()
        _hip.check(lib.gdt_crop_resize_workspace_bytes(max(n, 1), max(ow, 1), max(oh, 1), ctypes.byref(size)))
        return lib.gdt_crop_resize_u8_batch(arr if items else None, n, ow, oh, None, (ctypes.c_float * 3)(*std) if std else None, ws,
                                            size.value if ws_bytes is None else ws_bytes, None)

    for kwargs in (dict(n=0), dict(ow=0), dict(oh=-1), dict(src=None), dict(dst=None), dict(ws=None), dict(items=False), dict(box=(2, 1, 0, 18)), dict(box=(2, 1, 17, 0)),
                   dict(box=(-1, 1, 17, 18)), dict(box=(2, -1, 17, 18)), dict(box=(14, 1, 17, 18)), dict(box=(2, 1, 17, 20)), dict(box=(2, 3, 17, 18)), dict(h=0), dict(std=(0.5, 0.0, 0.5))):
        with pytest.raises(ValueError):
            _hip.check(call(**kwargs))
    assert call(ws_bytes=64) == _hip.GDT_ERR_WORKSPACE
    with pytest.raises(RuntimeError, match="workspace"):
        _hip.check(call(ws_bytes=64))
