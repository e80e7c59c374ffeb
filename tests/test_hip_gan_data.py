"""The GAN scenarios' data on the device: gdt_crop_resize_u8_batch against the float64 evaluation of its arithmetic (tests/crop_resize_ref.py), its
identity-table form and the LANCZOS path bit for bit, the loaders of the published data blocks end to end, and ``step_losses`` on a loader batch.

Gate of the bilinear cases, per element: |got - ref| <= 4 * 2**-24 / std_c + 2**-22 * |ref| -- three fp32 roundings (two products, one sum) of the
horizontal and of the vertical blend on values in [0, 1] (2**-25 each at most, the first three scaled by weights that sum to one), one rounding each for
the subtraction of the mean and the IEEE division.  Derived, not measured; every case prints its largest error over gate.

Measured on an MI355X, largest |got - ref| / gate per case: 0.19 .. 0.36 on the bilinear cases (0.36: three items with ``flip_dst``), 0 on the
all-zero boxes; every bit-exact case equal."""
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

pytestmark = pytest.mark.gpu

MEAN_STD = [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]]
UNEVEN = [[0.485, 0.456, 0.406], [0.229, 0.224, 0.225]]
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gan_data.npz"))


def _check(dev, images, boxes, ow, oh, flips=None, mean_std=None):
    from gandtr_amd import ingest
    got = ingest.crop_resize([torch.from_numpy(img).to(dev) for img in images], boxes, ow, oh, flips, mean_std)
    assert got.shape == (len(images), 3, oh, ow) and got.dtype == torch.float32 and got.device == dev
    got = got.cpu().numpy().astype(np.float64)
    mean, std = mean_std if mean_std is not None else (None, None)
    worst = 0.0
    for i, (img, box) in enumerate(zip(images, boxes)):
        fs, fd = flips[i] if flips is not None else (False, False)
        ref = REF.crop_resize(img, box, ow, oh, fs, fd, mean, std)
        ratio = np.abs(got[i] - ref) / REF.gate(ref, std)
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), (i, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
    print("largest |got - ref| / gate = %.3f" % worst)
    return got


def test_unaligned_rows_and_both_clamps(cuda_device):
    """16 x 16 from a 17 x 20 box at an odd x0: row starts at every byte alignment, the first and last output columns / rows clamp"""
    _check(cuda_device, [FX.photo(1, 40, 50)], [(3, 7, 17, 20)], 16, 16, mean_std=UNEVEN)


def test_tail_lanes(cuda_device):
    """out_w = 18 is no multiple of 4: scalar stores, a partial last lane"""
    _check(cuda_device, [FX.photo(2, 40, 50)], [(2, 5, 13, 29)], 18, 10, mean_std=UNEVEN)
    _check(cuda_device, [FX.photo(2, 40, 50)], [(0, 1, 40, 49)], 5, 7, mean_std=MEAN_STD)
    _check(cuda_device, [FX.photo(2, 40, 50)], [(1, 0, 3, 2)], 1, 1, mean_std=MEAN_STD)


def test_nothing_outside_the_box_is_read(cuda_device):
    """pixels outside the box are 255, inside 0: a tap clamped to the image instead of the box would show.  One box touches the right / bottom edge,
    one lies in the middle"""
    img = np.full((30, 40, 3), 255, dtype=np.uint8)
    img[10:30, 15:40] = 0
    got = _check(cuda_device, [img], [(10, 15, 20, 25)], 16, 16, mean_std=UNEVEN)
    assert (got < 0).all()
    img = np.full((30, 40, 3), 255, dtype=np.uint8)
    img[5:22, 9:30] = 0
    for flips in ([(False, False)], [(True, False)], [(False, True)]):
        assert (_check(cuda_device, [img], [(5, 9, 17, 21)], 16, 12, flips) == 0).all()


def test_whole_image_and_two_to_one(cuda_device):
    _check(cuda_device, [FX.photo(3, 23, 31)], [(0, 0, 23, 31)], 16, 16, mean_std=MEAN_STD)
    _check(cuda_device, [FX.photo(4, 32, 32)], [(0, 0, 32, 32)], 16, 16, mean_std=MEAN_STD)


def test_more_than_one_block_per_row_and_column(cuda_device):
    """out_w > 256: two blocks in x; the published geometry: 256 x 256 from a 300 x 320 box"""
    _check(cuda_device, [FX.photo(5, 24, 400)], [(1, 3, 20, 390)], 300, 6, mean_std=MEAN_STD)
    _check(cuda_device, [FX.photo(6, 330, 411)], [(11, 60, 300, 320)], 256, 256, mean_std=MEAN_STD)


def test_three_items_of_different_sizes_with_flips_in_one_call(cuda_device):
    images = [FX.photo(7, 40, 50), FX.photo(8, 25, 64), FX.photo(9, 61, 33)]
    boxes = [(3, 7, 17, 20), (0, 0, 25, 64), (20, 10, 41, 23)]
    plain = _check(cuda_device, images, boxes, 16, 16, mean_std=UNEVEN)
    src = _check(cuda_device, images, boxes, 16, 16, [(True, False)] * 3, UNEVEN)
    dst = _check(cuda_device, images, boxes, 16, 16, [(False, True)] * 3, UNEVEN)
    both = _check(cuda_device, images, boxes, 16, 16, [(False, False), (True, True), (False, True)], UNEVEN)
    assert np.array_equal(dst, plain[..., ::-1]) and not np.array_equal(src, plain)
    assert np.array_equal(both[0], plain[0]) and np.array_equal(both[1], src[1][..., ::-1]) and np.array_equal(both[2], dst[2])


def test_null_mean_std_is_the_unit_image(cuda_device):
    got = _check(cuda_device, [FX.photo(10, 40, 50)], [(3, 7, 17, 20)], 16, 16)
    assert got.min() >= 0.0 and got.max() <= 1.0


def _normalised(u8, mean_std):
    """``totensor | normalize`` by torch on the CPU in float32"""
    x = torch.from_numpy(np.asarray(u8).copy(order="C")).permute(2, 0, 1).float() / 255
    if mean_std is None:
        return x
    return (x - torch.tensor(mean_std[0])[:, None, None]) / torch.tensor(mean_std[1])[:, None, None]


@pytest.mark.parametrize("mean_std", [None, MEAN_STD, UNEVEN], ids=["unit", "half", "uneven"])
def test_identity_tables_are_bit_exact(cuda_device, mean_std):
    from gandtr_amd import ingest
    img = FX.photo(11, 40, 50)
    for (y0, x0, ch, cw) in [(3, 7, 16, 20), (0, 0, 40, 50), (39, 49, 1, 1), (5, 1, 30, 17)]:
        for fs, fd in ((False, False), (True, False), (False, True)):
            got = ingest.crop_resize([torch.from_numpy(img).to(cuda_device)], [(y0, x0, ch, cw)], cw, ch, [(fs, fd)], mean_std)[0].cpu()
            crop = img[y0:y0 + ch, x0:x0 + cw]
            assert torch.equal(got, _normalised(crop[:, ::-1] if fs or fd else crop, mean_std)), ((y0, x0, ch, cw), fs, fd)


@pytest.mark.parametrize("chain,shapes", [("center_crop:16_12", [(21, 33), (13, 16)]), ("square_crop", [(30, 20), (17, 17)]),
                                          ("scalecrop:24_16:0.8_1", [(16, 24)]), ("square_crop | mirror:1", [(20, 33)])])
def test_crops_through_apply_many_are_bit_exact(cuda_device, chain, shapes):
    from gandtr_amd.ingest import DeviceTransform
    from gandtr_amd.components.data import transform as T
    pics = [FX.photo(20 + i, h, w) for i, (h, w) in enumerate(shapes)]
    transform = DeviceTransform("pil2np | %s | totensor | normalize" % chain, UNEVEN)
    columns = transform.apply_many([[torch.from_numpy(p).to(cuda_device) for p in pics]], [transform.plan(shapes)])
    host = T.initialize_transforms("pil2np | %s | totensor | normalize" % chain, UNEVEN)(*pics)
    host = [host] if len(pics) == 1 else host
    assert len(columns) == len(pics)
    for col, pic, want in zip(columns, pics, host):
        assert col.shape[0] == 1 and torch.equal(col[0].cpu(), want)


@pytest.mark.parametrize("name", sorted(FX.DOWNSCALE_CASES))
def test_downscale_is_pillows(cuda_device, name):
    from gandtr_amd.ingest import DeviceTransform
    (h, w), n = FX.DOWNSCALE_CASES[name]
    transform = DeviceTransform("pil2np | downscale:%d | totensor | normalize" % n, MEAN_STD)
    img = torch.from_numpy(FX.photo(11, h, w)).to(cuda_device)
    col, = transform.apply_many([[img]], [transform.plan([(h, w)])])
    want = (torch.from_numpy(GOLD[name]).permute(2, 0, 1) - 0.5) / 0.5
    assert torch.equal(col[0].cpu(), want)
    mirrored = DeviceTransform("pil2np | downscale:%d | mirror:1 | totensor | normalize" % n, MEAN_STD)
    col, = mirrored.apply_many([[img]], [mirrored.plan([(h, w)])])
    assert torch.equal(col[0].cpu(), want.flip(2))


def test_apply_clahe_after_geometry(cuda_device):
    from gandtr_amd import clahe, ingest
    transform = ingest.DeviceTransform("pil2np | centerscalecrop:64_64:0.8 | apply_clahe:1.0 | totensor | normalize", MEAN_STD)
    img = torch.from_numpy(FX.photo(12, 90, 100)).to(cuda_device)
    plan = transform.plan([(90, 100)])
    col, = transform.apply_many([[img]], [plan])
    unit = ingest.crop_resize([img], [plan[0].box], 64, 64)
    assert col.shape == (1, 3, 64, 64) and torch.equal(col, clahe.clahe_lab(unit, 1.0, 8, None, MEAN_STD))


# ---- the loaders of the published data blocks ----

X_SHAPES, Y_SHAPES = [(300, 411), (257, 256), (290, 300)], [(280, 500), (320, 320), (256, 256)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("gan_data")
    for dom, shapes in (("X", X_SHAPES), ("Y", Y_SHAPES)):
        for i, (h, w) in enumerate(shapes):
            Image.fromarray(FX.photo(30 + i, h, w)).save(str(root / ("%s%d.jpg" % (dom, i))), quality=90)
        (root / (dom + ".txt")).write_text("".join("%s%d.jpg\n" % (dom, i) for i in range(len(shapes))))
    Image.fromarray(FX.photo(40, 300, 300)).save(str(root / "P0.png"))
    for i in range(2):
        Image.fromarray(FX.photo(41 + i, 400, 724)).save(str(root / ("V%d.%s" % (i, "png" if i else "jpg"))), quality=90)
    with open(str(root / "val.pkl"), "wb") as f:
        pickle.dump({"val": [["X0.jpg", "Y0.jpg"], ["X1.jpg", "Y1.jpg"], ["X2.jpg", "P0.png"]]}, f)
    return root


def pil_loader(data):
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _train_block(files, batch_size, size=6):
    """parameters/_gan_data.yml, ``train`` (paths, epoch size and batch size are the test's)"""
    return {"dataset": {"name": "RandomDomainsPair", "dataset_X": str(files / "X.txt"), "dataset_Y": str(files / "Y.txt"), "image_dir": str(files) + "/*", "size": size},
            "loader": {"batch_size": batch_size}, "transforms": "pil2np | scalecrop:256_256:0.8_1 | totensor | normalize",
            "mean_std": [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]]}


def _val_block(files, batch_size):
    """parameters/_gan_data.yml, ``val``"""
    return {"dataset": {"name": "PregeneratedImageTuple", "image_dir": str(files) + "/*", "dataset": str(files / "val.pkl"), "data_key": "val", "idx": "0_1"},
            "loader": {"batch_size": batch_size}, "transforms": "pil2np | totensor | normalize", "mean_std": [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]]}


@pytest.mark.parametrize("batch_size", [1, 3])
def test_train_loader(cuda_device, files, batch_size):
    from gandtr_amd.components.data import dataset as D

    def epoch():
        loader = D.initialize_dataset_loader(None, "train", _train_block(files, batch_size), device=cuda_device)
        np.random.seed(4)
        loader.dataset.prepare_epoch(None, None)
        random.seed(9)
        return loader, list(loader)
    loader, first = epoch()
    assert len(loader) == 6 // batch_size == len(first)
    for batch in first:
        assert isinstance(batch, list) and len(batch) == 2
        assert all(t.shape == (batch_size, 3, 256, 256) and t.dtype == torch.float32 and t.device == cuda_device for t in batch)
        assert all(float(t.min()) >= -1 and float(t.max()) <= 1 for t in batch)
    _, second = epoch()
    assert all(torch.equal(a, b) for x, y in zip(first, second) for a, b in zip(x, y))


def test_train_batch_is_apply_many_with_the_reference_boxes(cuda_device, files):
    """item (X0, Y0) has the shapes of the fixture's ``sc256_pair``: under ``random.seed(k)`` the loader's batch is the crop-resize of the recorded box"""
    from gandtr_amd import jpeg
    from gandtr_amd.components.data import dataset as D
    from gandtr_amd.ingest import Geometry
    loader = D.initialize_dataset_loader(None, "train", _train_block(files, 1, size=1), device=cuda_device)
    loader.dataset.idxs_X, loader.dataset.idxs_Y = [0], [0]
    decoded = jpeg.load_many([str(files / "X0.jpg"), str(files / "Y0.jpg")], cuda_device)
    assert [tuple(t.shape[:2]) for t in decoded] == [X_SHAPES[0], Y_SHAPES[0]]
    for row in (0, 3, 7):
        random.seed(FX.SEEDS[row])
        batch, = list(loader)
        boxes = [tuple(int(v) for v in GOLD["sc256_pair_box"][row, pic]) for pic in range(2)]
        plans = [[Geometry(box, False, ("bilinear", 256, 256), False, (256, 256)) for box in boxes]]
        want = loader.dataset.transform.apply_many([decoded], plans)
        assert all(torch.equal(a, b) for a, b in zip(batch, want))
        for pic in range(2):
            ref = REF.crop_resize(decoded[pic].cpu().numpy(), boxes[pic], 256, 256, mean=MEAN_STD[0], std=MEAN_STD[1])
            assert (np.abs(batch[pic][0].cpu().numpy().astype(np.float64) - ref) <= REF.gate(ref, MEAN_STD[1])).all()


def test_val_loader_and_the_png_fallback(cuda_device, files):
    from gandtr_amd import jpeg
    from gandtr_amd.components.data import dataset as D
    with pytest.raises(ValueError):
        list(D.initialize_dataset_loader(None, "val", _val_block(files, 1), device=cuda_device))          # the PNG, without a loader
    loader = D.initialize_dataset_loader(None, "val", _val_block(files, 1), loader_default_params={"loader": pil_loader}, device=cuda_device)
    batches = list(loader)
    assert len(loader) == 3 and [[tuple(t.shape) for t in b] for b in batches] == [[(1, 3, *X_SHAPES[i]), (1, 3, *s)] for i, s in
                                                                                   enumerate([Y_SHAPES[0], Y_SHAPES[1], (300, 300)])]
    assert torch.equal(batches[2][1][0].cpu(), _normalised(FX.photo(40, 300, 300), MEAN_STD))
    decoded = jpeg.load_many([str(files / "X1.jpg")], cuda_device)[0].cpu().numpy()
    assert torch.equal(batches[1][0][0].cpu(), _normalised(decoded, MEAN_STD))
    assert all(torch.equal(a, b) for x, y in zip(batches, list(loader)) for a, b in zip(x, y))
    with pytest.raises(RuntimeError, match="equal size"):
        list(D.initialize_dataset_loader(None, "val", _val_block(files, 3), loader_default_params={"loader": pil_loader}, device=cuda_device))


@pytest.mark.parametrize("batch_size", [1, 3])
def test_visual_loader(cuda_device, files, batch_size):
    """parameters/_gan_eval.yml, ``visual.criterion.data``"""
    from PIL import Image
    from gandtr_amd.components.data import dataset as D
    params = {"dataset": {"name": "InferImageList", "image_dir": str(files) + "/*"}, "transforms": "pil2np | downscale:362 | totensor | normalize",
              "mean_std": [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]]}
    loader = D.initialize_dataset_loader([["V0.jpg", "V1.png"]], "test", params, loader_default_params={"batch_size": batch_size, "loader": pil_loader},
                                         device=cuda_device)
    batches = list(loader)
    assert len(batches) == len(loader) == (2 if batch_size == 1 else 1)
    names = [n for b in batches for n in b[0][0]]
    images = torch.cat([b[1] for b in batches])
    assert names == ["V0.jpg", "V1.png"] and images.shape == (2, 3, 200, 362) and images.device == cuda_device
    thumb = Image.fromarray(FX.photo(42, 400, 724))
    thumb.thumbnail((362, 362), Image.LANCZOS)
    assert torch.equal(images[1].cpu(), _normalised(np.asarray(thumb), MEAN_STD))


def test_step_losses_on_a_loader_batch(cuda_device, files):
    """SupervisedCycleGanEpoch on what the train loader yields (16 x 16 crops, small synthetic networks): finite values under the reference's keys"""
    import gan_objective_fixture as OFX
    from gandtr_amd.components.data import dataset as D
    from gandtr_amd.components.model.network import p2p_networks
    from gandtr_amd.tools import synth
    block = _train_block(files, 2, size=2)
    block["transforms"] = "pil2np | scalecrop:16_16:0.8_1 | totensor | normalize"
    loader = D.initialize_dataset_loader(None, "train", block, device=cuda_device)
    np.random.seed(1)
    loader.dataset.prepare_epoch(None, None)
    random.seed(1)
    (X, Y), = list(loader)
    assert X.shape == Y.shape == (2, 3, 16, 16)

    def gen(seed):
        net = p2p_networks.ResnetGenerator(3, 3, ngf=16, norm_layer="instance", n_blocks=3).eval()
        net.load_state_dict(synth.generator_state(seed, "instance", ngf=16, n_blocks=3))
        return net.to(cuda_device)

    def disc(seed):
        net = p2p_networks.NLayerDiscriminator(3, ndf=16, n_layers=2, norm_layer="instance").eval()
        net.load_state_dict(synth.discriminator_state(seed, "instance", ndf=16, n_layers=2, gain=0.2))
        return net.to(cuda_device)
    nets = {"generator_X": gen(0), "generator_Y": gen(1), "discriminator_X": disc(40), "discriminator_Y": disc(41)}
    losses, _ = OFX.mirror_epoch("SupervisedCycleGanEpoch").step_losses(nets, X, Y)
    assert list(losses) == [str(k) for k in OFX.gold()["cyclegan_0_keys"]]          # the reference's keys, in its order
    assert all(np.isfinite(v) for v in losses.item().values())
