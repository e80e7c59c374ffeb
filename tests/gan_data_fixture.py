"""Cases of tests/golden/gan_data.npz, shared by its generator (tests/golden/make_gan_data_golden.py, which runs the reference's transforms and datasets on
them) and its consumers (tests/test_gan_data_host.py, tests/test_hip_gan_data.py).  Inputs are regenerated from seeds here; the file holds results only."""
import numpy as np

SEEDS = tuple(range(10))

# name -> (chain of geometric steps, (h, w) of the item's pics).  Under ``random.seed(k)`` the reference's Compose of the chain runs on the pics; recorded
# per seed: per pic the source box (y0, x0, ch, cw) in the unmirrored pic (the whole pic when it came back unchanged), whether it was mirrored before /
# after the resize, whether it was resized; ``random.random()`` drawn right after (pins how many numbers the chain drew); 1 where the reference's own
# assert refused the item.
CROP_CASES = {
    "sc256_wide": ("scalecrop:256_256:0.8_1", [(300, 411)]),
    "sc256_one_row_more": ("scalecrop:256_256:0.8_1", [(257, 256)]),
    "sc256_pair": ("scalecrop:256_256:0.8_1", [(300, 411), (280, 500)]),
    "sc256_shortcut": ("scalecrop:256_256:0.8_1", [(256, 256)]),
    "sc256_shortcut_pair": ("scalecrop:256_256:0.8_1", [(256, 256), (256, 256)]),
    "sc256_no_shortcut_pair": ("scalecrop:256_256:0.8_1", [(256, 256), (300, 300)]),
    "sc16_default_scale": ("scalecrop:16_16", [(37, 53)]),
    "sc16_pair": ("scalecrop:16_16:0.8_1", [(37, 53), (20, 45)]),
    "sc24x16": ("scalecrop:24_16:0.8_1", [(30, 40)]),
    "sc24x16_unreversed_assert": ("scalecrop:24_16:0.8_1", [(20, 45)]),          # the crop would fit; size (w, h) is compared with (h, w)
    "csc256": ("centerscalecrop:256_256:0.8", [(300, 411)]),
    "csc256_pair": ("centerscalecrop:256_256:0.8", [(330, 411), (321, 500)]),
    "csc16_default_scale": ("centerscalecrop:16_16", [(37, 53)]),
    "csc24x16": ("centerscalecrop:24_16:0.8", [(30, 40)]),
    "csc256_shortcut": ("centerscalecrop:256_256:0.8", [(256, 256)]),
    "sc256_then_mirror": ("scalecrop:256_256:0.8_1 | mirror", [(300, 411), (280, 500)]),
    "mirror_then_sc16": ("mirror | scalecrop:16_16:0.8_1", [(37, 53)]),
    "mirror_sc16_mirror": ("mirror:0.7 | scalecrop:16_16:0.8_1 | mirror:0.3", [(37, 53)]),
    "center_crop_even": ("center_crop:16_12", [(20, 30)]),
    "center_crop_odd": ("center_crop:16_12", [(21, 33), (13, 16)]),
    "square_crop_wide_odd": ("square_crop", [(20, 33)]),
    "square_crop_tall_even": ("square_crop", [(30, 20), (17, 17)]),
    "square_then_csc16": ("square_crop | centerscalecrop:16_16:0.8", [(37, 53)]),
}

# Downscale (Pillow's LANCZOS thumbnail through the float -> uint8 -> float round trip): (h, w) -> N
DOWNSCALE_CASES = {"down_37x53": ((37, 53), 16), "down_16x16": ((16, 16), 16), "down_53x37": ((53, 37), 16)}

# RandomDomainsPair.prepare_epoch: (len X, len Y, size, numpy seed)
PAIR_CASES = {"pairs_a": (7, 5, 11, 0), "pairs_b": (3, 9, 4, 5)}

# PregeneratedImageTuple: tuple lengths of the pickled list, idx strings
TUPLE_LENGTHS = (2, 5, 3, 4, 2, 6)
TUPLE_IDX = ("0_1", "0_any", "0_different", "-1_different_any")


def coordinate_pic(h, w):
    """float32 h x w x 3: channel 0 = y * w + x, channel 1 = w, channel 2 = 0 -- a slice or mirror of it tells where it came from"""
    pic = np.zeros((h, w, 3), dtype=np.float32)
    pic[..., 0] = np.arange(h * w, dtype=np.float32).reshape(h, w)
    pic[..., 1] = w
    return pic


def photo(seed, h, w):
    """uint8 h x w x 3 test image: smooth structure plus noise, the full 0..255 range"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 127.5 + 100 * np.sin(x / 5.0 + seed) * np.cos(y / 7.0)
    img = base[..., None] + rng.normal(0, 30, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def tuple_names():
    return [["t%d_%d.jpg" % (i, j) for j in range(n)] for i, n in enumerate(TUPLE_LENGTHS)]
