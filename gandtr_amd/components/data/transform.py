"""CPU image preprocessing attached to hub models as ``.transform`` -- host mirror of
mdir/components/data/transform/__init__.py:37-46 (initialize_transforms), core_transforms.py:25-100
(Compose, ToTensor, Normalize, Pil2Numpy) and photometric_transforms.py:28-36 / functional.py:140-161 (ApplyClahe).
Host-side only (out of the HIP scope); CLAHE needs opencv and raises ImportError without it.
The geometric steps of the GAN scenarios' data (augmentation_transforms.py:24-164: mirror, center_crop, square_crop, downscale, scalecrop,
centerscalecrop) run without opencv: the bilinear step is a numpy restatement of cv2's INTER_LINEAR float path."""
import math
import random

import numpy as np
import torch


class GenericTransform:
    def __init__(self, params=None):
        self.params = params or {}

    def __repr__(self):
        return type(self).__name__ + "(%s)" % ", ".join("%s=%s" % kv for kv in self.params.items())


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, *pics):
        for t in self.transforms:
            pics = t(*pics)
        return pics[0] if len(pics) == 1 else pics

    def __repr__(self):
        return type(self).__name__ + "(" + "".join("\n    %s" % t for t in self.transforms) + "\n)"


class Pil2Numpy(GenericTransform):
    """PIL image / ndarray -> float32 HWC array in [0, 1]"""

    def __call__(self, *pics):
        out = []
        for pic in pics:
            if hasattr(pic, "convert"):
                pic = np.asarray(pic.convert("RGB"))
            elif not isinstance(pic, np.ndarray):
                raise ValueError("Unsupported type '%s'" % type(pic))
            if pic.dtype == np.uint8:
                pic = pic.astype(np.float32) / 255.0
            elif pic.dtype == np.uint16:
                pic = pic.astype(np.float32) / 65535.0
            else:
                pic = pic.astype(np.float32)
            out.append(pic)
        return out


class ImageClahe:
    """CLAHE on the L channel of LAB (8-bit quantised), cv2-based as in the reference (functional.py:140-161)."""

    def __init__(self, clip_limit, grid_size, colorspace="lab"):
        self.clip_limit, self.grid_size, self.colorspace = clip_limit, grid_size, colorspace

    def apply(self, img):
        if isinstance(img, torch.Tensor) and img.is_cuda:       # H x W x 3 on a HIP device: gandtr_amd/csrc/clahe.hip
            if self.colorspace != "lab":
                raise NotImplementedError("only the 'lab' colorspace is supported")
            from ... import clahe
            return clahe.clahe_lab(img.permute(2, 0, 1)[None], self.clip_limit, self.grid_size)[0].permute(1, 2, 0)
        try:
            import cv2
        except ImportError as e:          # pragma: no cover - depends on the image
            raise ImportError("CLAHE preprocessing needs opencv-python (cv2), which is not installed") from e
        if self.colorspace != "lab":
            raise NotImplementedError("only the 'lab' colorspace is supported")
        lab = cv2.cvtColor(img.astype(np.float32), cv2.COLOR_RGB2LAB)
        clahe = cv2.createCLAHE(clipLimit=self.clip_limit, tileGridSize=(self.grid_size, self.grid_size))
        chan = (lab[..., 0] / 100.0 * 255).astype(np.uint8)
        lab[..., 0] = clahe.apply(chan).astype(np.float32) / 255.0 * 100.0
        return cv2.cvtColor(lab, cv2.COLOR_LAB2RGB)


class ApplyClahe(GenericTransform):
    def __init__(self, clip_limit, grid_size=8, colorspace="lab"):
        super().__init__({"clip_limit": float(clip_limit), "grid_size": int(grid_size), "colorspace": colorspace})
        self.clahe = ImageClahe(**self.params)

    def __call__(self, *pics):
        return [self.clahe.apply(p) for p in pics]


class ToTensor(GenericTransform):
    """HWC float array -> CHW tensor (uint8 input is scaled to [0, 1], like torchvision's ToTensor)"""

    def __call__(self, *pics):
        out = []
        for pic in pics:
            pic = np.asarray(pic)
            if pic.ndim == 2:
                pic = pic[:, :, None]
            t = torch.from_numpy(np.ascontiguousarray(pic.transpose((2, 0, 1))))
            out.append(t.float().div(255) if t.dtype == torch.uint8 else t)
        return out


class Normalize(GenericTransform):
    def __init__(self, mean, std, strict_shape=True):
        if isinstance(strict_shape, str):
            strict_shape = strict_shape.lower() != "false"
        super().__init__({"mean": mean, "std": std, "strict_shape": bool(strict_shape)})
        assert len(mean) == len(std)

    def __call__(self, *pics):
        out = []
        for pic in pics:
            n = pic.size(0)
            if self.params["strict_shape"]:
                assert n == len(self.params["mean"]), (n, len(self.params["mean"]))
            else:
                assert n <= len(self.params["mean"]), (n, len(self.params["mean"]))
            mean = torch.as_tensor(self.params["mean"][:n], dtype=pic.dtype)[:, None, None]
            std = torch.as_tensor(self.params["std"][:n], dtype=pic.dtype)[:, None, None]
            out.append((pic - mean) / std)
        return out


#
# Crop, scale and flip: the steps ``mirror``, ``center_crop``, ``square_crop``, ``downscale``, ``scalecrop`` and ``centerscalecrop`` of the reference's
# chains, written from the behaviour tests/golden/gan_data.npz records of its classes.  Every class states its geometry ONCE, in ``ops(shapes, rng)``:
# per pic one of None (unchanged), ("crop", y0, x0, ch, cw), ("flip",), ("bilinear", y0, x0, ch, cw, ow, oh) or ("lanczos", n), asking ``rng`` for
# exactly the numbers the reference asks ``random`` for, in its order, so that ``random.seed(s)`` reproduces its crops.  ``__call__`` applies the ops to
# numpy pics; gandtr_amd.ingest.DeviceTransform.plan composes the same ops into one source box + flips + resampler per pic for the device.
#

def parse_tuple(text, dtype=int):
    """"256_256" -> (256, 256); anything that is not a string is taken as the tuple it already is"""
    return tuple(dtype(part) for part in text.split("_")) if isinstance(text, str) else tuple(text)


def linear_taps(n_in, n_out):
    """cv2's INTER_LINEAR float path for one axis (what ``cv2.resize`` of a float32 image computes): per output index the two source taps and the fp32
    weight of the second.  The coordinate is formed in double and CAST TO float32 before the floor, the clamps are to the source extent."""
    d = np.arange(n_out, dtype=np.float64)
    f = ((d + 0.5) * (n_in / float(n_out)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    low, high = s < 0, s >= n_in - 1
    s[low], f[low] = 0, 0
    s[high], f[high] = n_in - 1, 0
    return s, np.minimum(s + 1, n_in - 1), f.astype(np.float32)


def bilinear_resize(pic, out_w, out_h):
    """``cv2.resize(pic, (out_w, out_h))`` for a float32 H x W [x C] array, restated in numpy (cv2 is not a dependency): the horizontal blend first, then
    the vertical one, in fp32 with the weights ``1.f - f`` and ``f``"""
    pic = np.asarray(pic, dtype=np.float32)
    sx0, sx1, fx = linear_taps(pic.shape[1], out_w)
    sy0, sy1, fy = linear_taps(pic.shape[0], out_h)
    tail = (1,) * (pic.ndim - 2)
    fx, fy = fx.reshape((1, -1) + tail), fy.reshape((-1, 1) + tail)
    rows = pic[:, sx0] * (np.float32(1) - fx) + pic[:, sx1] * fx
    return rows[sy0] * (np.float32(1) - fy) + rows[sy1] * fy


class GeometricTransform(GenericTransform):
    def __init__(self, **params):
        super().__init__(params)

    def ops(self, shapes, rng):
        raise NotImplementedError

    def __call__(self, *pics):
        if not all(isinstance(p, np.ndarray) for p in pics):
            raise RuntimeError("%s works on numpy pics (put pil2np first), got %s" % (type(self).__name__, [type(p).__name__ for p in pics]))
        ops = self.ops([p.shape[:2] for p in pics], random)
        if all(op is None for op in ops):
            return pics
        return [apply_op(p, op) for p, op in zip(pics, ops)]


def _thumbnail(pic, n):
    """Pillow's LANCZOS thumbnail of a float [0, 1] pic: quantised to 8 bits by truncation on the way in, back to float32 / 255 on the way out"""
    from PIL import Image
    image = Image.fromarray((pic * 255).astype(np.uint8))
    image.thumbnail((n, n), Image.LANCZOS)
    return np.asarray(image).astype(np.float32) / 255.0


def apply_op(pic, op):
    if op is None:
        return pic
    kind, args = op[0], op[1:]
    if kind == "flip":
        return np.ascontiguousarray(pic[:, ::-1])
    if kind == "lanczos":
        return _thumbnail(pic, args[0])
    y0, x0, ch, cw = args[:4]
    crop = pic[y0:y0 + ch, x0:x0 + cw]
    if kind == "crop":
        return crop
    if kind == "bilinear":
        return bilinear_resize(crop, args[4], args[5])
    raise ValueError(op)


class RandomHorizontalFlip(GeometricTransform):
    """with probability ``p`` (one ``rng.random()`` per item) all pics of the item are mirrored left-right"""

    def __init__(self, p=0.5):
        super().__init__(p=float(p))

    def ops(self, shapes, rng):
        flip = rng.random() < self.params["p"]
        return [("flip",) if flip else None for _ in shapes]


def _centred(extent, wanted):
    """first index of ``wanted`` centred pixels out of ``extent``: an odd surplus leaves the extra pixel at the far end"""
    return (extent - wanted) // 2


class CenterCrop(GeometricTransform):
    """``center_crop:W_H``: the middle H x W pixels of every pic"""

    def __init__(self, size):
        w, h = parse_tuple(size, int)
        super().__init__(size=np.array([h, w]))

    def ops(self, shapes, rng):
        h, w = (int(v) for v in self.params["size"])
        for shape in shapes:
            if shape[0] < h or shape[1] < w:
                raise ValueError("center_crop: a %d x %d pic is smaller than the %d x %d crop" % (shape[0], shape[1], h, w))
        return [("crop", _centred(shape[0], h), _centred(shape[1], w), h, w) for shape in shapes]


class SquareCrop(GeometricTransform):
    """``square_crop``: the middle square of every pic, its side the pic's shorter one"""

    def ops(self, shapes, rng):
        acc = []
        for h, w in shapes:
            side = min(h, w)
            acc.append(("crop", _centred(h, side), _centred(w, side), side, side))
        return acc


class Downscale(GeometricTransform):
    """``downscale:N``: pics whose longer side exceeds N are shrunk to fit N x N, aspect kept (Pillow's LANCZOS thumbnail, as the reference does it)"""

    def __init__(self, size):
        super().__init__(size=int(size))

    def ops(self, shapes, rng):
        n = self.params["size"]
        return [("lanczos", n) if max(shape) > n else None for shape in shapes]


class RandomScaleCrop(GeometricTransform):
    """``scalecrop:W_H[:lo_hi]``: a random crop of a randomly scaled pic, done as ONE crop of H / s x W / s pixels (rounded up) resized to W x H, with
    s = lowest + u * (hi - lowest), u = ``rng.random()``, and lowest = the larger of ``lo`` and the scale at which the crop still fits.  The crop is
    placed by ``rng.randint`` (row first, then column) within the SMALLEST extents over the item's pics and shared by all of them.  Kept as the reference
    behaves: when the first two pics (or the only one) have equal shapes and that shape is the target, the item passes unchanged and nothing is drawn;
    the fit test and ``lowest`` compare W with the pics' height and H with their width."""

    def __init__(self, size, scale=(0.5, 0.8)):
        w, h = parse_tuple(size, int)
        low, high = parse_tuple(scale, float)
        super().__init__(size=np.array([w, h]), scale=(float(low), float(high)))

    def _untouched(self, shapes):
        w, h = (int(v) for v in self.params["size"])
        alike = len(shapes) == 1 or tuple(shapes[0]) == tuple(shapes[1])
        return alike and tuple(shapes[0]) == (h, w)

    def _scale(self, low, rng):
        return rng.random() * (self.params["scale"][1] - low) + low

    def _place(self, slack, rng):
        return rng.randint(0, slack)

    def ops(self, shapes, rng):
        if self._untouched(shapes):
            return [None] * len(shapes)
        w, h = (int(v) for v in self.params["size"])
        rows, cols = min(int(s[0]) for s in shapes), min(int(s[1]) for s in shapes)
        assert w <= rows and h <= cols, "target (%d, %d) against the smallest pic (%d, %d)" % (w, h, rows, cols)
        scale = self._scale(max(w / rows, h / cols, self.params["scale"][0]), rng)
        ch, cw = math.ceil(h / scale), math.ceil(w / scale)
        assert ch <= rows and cw <= cols, "a %d x %d crop does not fit %d x %d" % (ch, cw, rows, cols)
        y0 = self._place(rows - ch, rng)
        x0 = self._place(cols - cw, rng)
        return [("bilinear", y0, x0, ch, cw, w, h) for _ in shapes]


class CenterScaleCrop(RandomScaleCrop):
    """``centerscalecrop:W_H[:s]``: the same crop-and-resize at the fixed scale s, centred in the smallest extents; draws nothing"""

    def __init__(self, size, scale=0.6):
        super().__init__(size, (float(scale), float(scale)))

    def _scale(self, low, rng):
        return self.params["scale"][0]

    def _place(self, slack, rng):
        return slack // 2


TRANSFORMS = {"totensor": ToTensor, "normalize": Normalize, "pil2np": Pil2Numpy, "apply_clahe": ApplyClahe,
              "mirror": RandomHorizontalFlip, "center_crop": CenterCrop, "square_crop": SquareCrop, "downscale": Downscale,
              "scalecrop": RandomScaleCrop, "centerscalecrop": CenterScaleCrop}


def initialize_transforms(augmentations, mean_std):
    """'pil2np | apply_clahe:1.0 | totensor | normalize' -> Compose"""
    trans = []
    for aug in [x.strip() for x in augmentations.split("|") if x.strip()]:
        tname, *args = aug.split(":", 1)
        args = args[0].split(":") if args else []
        trans.append(TRANSFORMS[tname](*(list(mean_std) + args)) if "normalize" in aug else TRANSFORMS[tname](*args))
    return Compose(trans)
