"""Photometric transforms of the lightness channel -- mirror of mdir/components/data/transform/photometric_transforms.py:10-25,56-104
(AddClaheFromRgb, MatchHistogram, ReplaceChannelWithHistogram, GammaEqualize), channel_transforms.py:67-89 (AddIntensityFromRgb, ToColorspace) and
of the functions they call, functional.py:28-36,55-63,81-133.

H x W x C tensors on a HIP device go through gandtr_amd.photometric (gandtr_amd/csrc/photometric.hip), the way ``transform.ImageClahe.apply`` takes
device tensors to CLAHE.  numpy pics run the host path below, which needs neither cv2 nor scipy: the channel functions as functional.py:96-133 states
them, the secant iteration ``scipy.optimize.newton`` runs without ``fprime`` restated, and a float32 numpy Lab with OpenCV's constants (the direct CIE
formulas; cv2 itself goes through a spline and tables, so its floats differ in the low decimal places).  Only the "lab" colorspace is supported.

These names are NOT part of ``transform.TRANSFORMS``: ``initialize_transforms`` of this module resolves a chain in both registries."""
import warnings

import numpy as np
import torch

from ... import photometric as device
from . import transform
from .transform import GenericTransform

HISTOGRAM_BINS = device.HISTOGRAM_BINS
HISTOGRAM_CENTERS = device.HISTOGRAM_CENTERS

_F = np.float32
# OpenCV color_lab.cpp: sRGB D65 primaries and white point
_RGB2XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], np.float64)
_XYZ2RGB = np.array([[3.240479, -1.53715, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]], np.float64)
_WHITE = np.array([0.950456, 1.0, 1.088754], np.float64)
_FWD = (_RGB2XYZ / _WHITE[:, None]).astype(_F)
_INV = (_XYZ2RGB * _WHITE[None, :]).astype(_F)


def _require_lab(colorspace):
    if colorspace.lower() != "lab":
        raise NotImplementedError("Colorspace %s is not supported" % colorspace)


def _on_device(pic):
    return isinstance(pic, torch.Tensor) and pic.is_cuda


def _chw(pic):
    """H x W x 3 device tensor -> 1 x 3 x H x W"""
    return pic[:, :, :3].permute(2, 0, 1)[None]


#
# host Lab (float32)
#

def rgb2normspace(img, colorspace="lab"):
    """functional.py:28-36 for "lab": H x W x 3 float32 RGB in [0, 1] -> (L / 100, (a + 128) / 255, (b + 128) / 255)"""
    _require_lab(colorspace)
    c = np.clip(np.asarray(img, dtype=_F), _F(0), _F(1))
    lin = np.where(c <= _F(0.04045), c * _F(1.0 / 12.92), np.power((c + _F(0.055)) * _F(1.0 / 1.055), _F(2.4), dtype=_F)).astype(_F)
    xyz = [_FWD[i, 0] * lin[..., 0] + _FWD[i, 1] * lin[..., 1] + _FWD[i, 2] * lin[..., 2] for i in range(3)]
    f = [np.where(v > _F(0.008856), np.cbrt(v, dtype=_F), _F(7.787) * v + _F(16.0 / 116.0)).astype(_F) for v in xyz]
    L = np.where(xyz[1] > _F(0.008856), _F(116.0) * f[1] - _F(16.0), _F(903.3) * xyz[1]).astype(_F)
    lab = np.stack([L, _F(500.0) * (f[0] - f[1]), _F(200.0) * (f[1] - f[2])], axis=-1).astype(_F)
    return ((lab + np.array([0, 128, 128], _F)) / np.array([100.0, 255.0, 255.0], _F)).astype(_F)


def normspace2rgb(spc, colorspace="lab"):
    """functional.py:55-63 for "lab"; the linear RGB is clipped to [0, 1] before the transfer curve, as OpenCV does"""
    _require_lab(colorspace)
    lab = np.asarray(spc, dtype=_F) * np.array([100.0, 255.0, 255.0], _F) - np.array([0, 128, 128], _F)
    L, a, b = (lab[..., i].astype(_F) for i in range(3))
    y_lo, fy_hi = L / _F(903.3), (L + _F(16.0)) / _F(116.0)
    low = L <= _F(0.008856 * 903.3)
    y = np.where(low, y_lo, fy_hi * fy_hi * fy_hi).astype(_F)
    fy = np.where(low, _F(7.787) * y_lo + _F(16.0 / 116.0), fy_hi).astype(_F)
    f_thresh = _F(7.787 * 0.008856 + 16.0 / 116.0)
    x, z = (np.where(fv <= f_thresh, (fv - _F(16.0 / 116.0)) / _F(7.787), fv * fv * fv).astype(_F) for fv in (a / _F(500.0) + fy, fy - b / _F(200.0)))
    out = []
    for i in range(3):
        c = np.clip(_INV[i, 0] * x + _INV[i, 1] * y + _INV[i, 2] * z, _F(0), _F(1))
        out.append(np.where(c <= _F(0.0031308), c * _F(12.92), np.power(c, _F(1.0 / 2.4), dtype=_F) * _F(1.055) - _F(0.055)).astype(_F))
    return np.stack(out, axis=-1).astype(_F)


def apply_lightness_transform(img, colorspace, func):
    """functional.py:81-85"""
    spc = rgb2normspace(img, colorspace)
    spc[:, :, 0] = func(spc[:, :, 0])
    return normspace2rgb(spc, colorspace)


#
# host channel functions (functional.py:96-133)
#

def channel_histogram_matching(chan0, histogram):
    cdf0 = np.cumsum(np.histogram(chan0, HISTOGRAM_BINS)[0]) / chan0.size
    centers = HISTOGRAM_CENTERS
    mode, cdf = device.target_cdf(histogram)
    if mode == device.MODE_EQ:
        return np.interp(chan0, centers, cdf0 * centers[-1]).astype(np.float32)
    return np.interp(chan0, centers, np.interp(cdf0, cdf, centers)).astype(np.float32)


def channel2channel_histogram_matching(chan0, chan1):
    cdf0 = np.cumsum(np.histogram(chan0, HISTOGRAM_BINS)[0]) / chan0.size
    cdf1 = np.cumsum(np.histogram(chan1, HISTOGRAM_BINS)[0]) / chan1.size
    return np.interp(chan0, HISTOGRAM_CENTERS, np.interp(cdf0, cdf1, HISTOGRAM_CENTERS)).astype(np.float32)


def secant(func, x0, tol=1e-4, maxiter=50):
    """``scipy.optimize.newton(func, x0, tol=tol, maxiter=maxiter)`` without ``fprime``: its second start point, swap, update and
    ``|p - p1| <= tol`` stop; RuntimeError where it raises one (equal function values at different points, or no convergence)"""
    p0 = 1.0 * x0
    p1 = x0 * (1 + 1e-4)
    p1 += (1e-4 if p1 >= 0 else -1e-4)
    q0, q1 = func(p0), func(p1)
    if abs(q1) < abs(q0):
        p0, p1, q0, q1 = p1, p0, q1, q0
    p = p1
    for _ in range(maxiter):
        if q1 == q0:
            if p1 != p0:
                raise RuntimeError("Tolerance of %s reached" % (p1 - p0))
            return (p1 + p0) / 2.0
        if abs(q1) > abs(q0):
            p = (-q0 / q1 * p1 + p0) / (1 - q0 / q1)
        else:
            p = (-q1 / q0 * p0 + p1) / (1 - q1 / q0)
        if np.isclose(p, p1, rtol=0.0, atol=tol):
            return p
        p0, q0 = p1, q1
        p1 = p
        q1 = func(p1)
    raise RuntimeError("Failed to converge after %d iterations, value is %s." % (maxiter, p))


def gamma_of(channel, target):
    """the exponent ``channel_gamma_matching`` applies (functional.py:116-129)"""
    def func(gamma):
        return np.mean(np.power(channel, gamma)) - target
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        x0 = np.log(target) / np.log(np.mean(channel))
        try:
            solution = secant(func, x0, tol=1e-4, maxiter=50)
        except RuntimeError:
            solution = 0.1 if abs(func(0.1)) < abs(func(10)) else 10
    return np.clip(solution, 0.1, 10)


def channel_gamma_matching(channel, target):
    return np.power(channel, gamma_of(channel, target))


def image_histogram_matching(img, histogram, colorspace="lab"):
    return apply_lightness_transform(img, colorspace, lambda x: channel_histogram_matching(x, histogram))


def image_gamma_matching(img, target, colorspace="lab"):
    return apply_lightness_transform(img, colorspace, lambda x: channel_gamma_matching(x, target))


#
# transforms
#

class MatchHistogram(GenericTransform):
    """Convert input images to given colorspace and match its lightness channel histogram to given value."""

    def __init__(self, histogram, colorspace="lab"):
        super().__init__({"histogram": histogram, "colorspace": colorspace})
        _require_lab(colorspace)

    def __call__(self, *pics):
        hist = self.params["histogram"]
        return [device.match_histogram(_chw(x), hist)[0].permute(1, 2, 0) if _on_device(x) else image_histogram_matching(x, hist) for x in pics]


class ReplaceChannelWithHistogram(GenericTransform):
    """Add a channel to the first image which is its last channel transformed to have specific pixel histogram.  With a second image the histogram is
    that of its last channel, which is removed; without one the histogram is a constant."""

    def __init__(self, histogram, created_channel):
        super().__init__({"histogram": histogram, "created_channel": created_channel})
        assert created_channel in {"append", "replace"}

    def __call__(self, pic0, *pics):
        cat = (lambda parts: torch.cat(parts, dim=2)) if _on_device(pic0) else (lambda parts: np.concatenate(parts, axis=2))
        pic0_output = pic0[:, :, :-1] if self.params["created_channel"] == "replace" else pic0
        if len(pics) == 1:
            pic1 = pics[0]
            if _on_device(pic0):
                add_chan = device.match_channel_to(pic0[:, :, -1], pic1[:, :, -1])
            else:
                add_chan = channel2channel_histogram_matching(pic0[:, :, -1], pic1[:, :, -1])
            return cat((pic0_output, add_chan[:, :, None])), pic1[:, :, :-1]
        if _on_device(pic0):
            add_chan = device.match_channel(pic0[:, :, -1], self.params["histogram"])
        else:
            add_chan = channel_histogram_matching(pic0[:, :, -1], self.params["histogram"])
        return (cat((pic0_output, add_chan[:, :, None])),) + tuple(pics)


class GammaEqualize(GenericTransform):
    """Convert images to a defined colorspace and apply gamma to the lightness channel, so that mean is shifted to target value between zero and one."""

    def __init__(self, target, colorspace="lab"):
        target = float(target)
        super().__init__({"target": target, "colorspace": colorspace})
        assert target > 0 and target < 1, target
        _require_lab(colorspace)

    def __call__(self, *pics):
        target = self.params["target"]
        return [device.gamma_equalize(_chw(x), target)[0].permute(1, 2, 0) if _on_device(x) else image_gamma_matching(x, target) for x in pics]


class ToColorspace(GenericTransform):
    """Convert RGB pics to given colorspace."""

    def __init__(self, colorspace):
        super().__init__({"colorspace": colorspace})
        _require_lab(colorspace)

    def __call__(self, *pics):
        return [device.to_lab(_chw(pic))[0].permute(1, 2, 0) if _on_device(pic) else rgb2normspace(pic[:, :, :3]) for pic in pics]


class AddIntensityFromRgb(GenericTransform):
    """Add a lightness channel from its rgb channels"""

    def __init__(self, colorspace="lab"):
        super().__init__({"colorspace": colorspace})
        _require_lab(colorspace)

    def __call__(self, *pics):
        acc = []
        for pic in pics:
            if _on_device(pic):
                acc.append(torch.cat((pic, device.lightness(_chw(pic))[0][:, :, None]), dim=2))
            else:
                assert isinstance(pic, np.ndarray)
                acc.append(np.concatenate((pic, rgb2normspace(pic[:, :, :3])[:, :, :1]), axis=2))
        return acc


class AddClaheFromRgb(GenericTransform):
    """Add a channel that is image's clahe-normalized lightness taken from its rgb channels.  On the device the quantised plane goes through
    ``clahe.clahe_u8``; numpy pics need opencv for the CLAHE itself, as ``transform.ImageClahe`` does."""

    def __init__(self, clip_limit=4, grid_size=8, colorspace="lab"):
        super().__init__({"clip_limit": float(clip_limit), "grid_size": int(grid_size), "colorspace": colorspace})
        _require_lab(colorspace)

    def __call__(self, *pics):
        acc = []
        for pic in pics:
            if _on_device(pic):
                from ... import clahe
                plane = (device.lightness(_chw(pic))[0] * 255).to(torch.uint8)                      # (chan * 255).astype(np.uint8), functional.py:148
                levels = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(pic.device)     # numpy's float32 quotients, bit for bit
                chan = levels[clahe.clahe_u8(plane, self.params["clip_limit"], self.params["grid_size"]).long()]
                acc.append(torch.cat((pic, chan[:, :, None]), dim=2))
                continue
            assert isinstance(pic, np.ndarray)
            try:
                import cv2
            except ImportError as e:          # pragma: no cover - depends on the image
                raise ImportError("CLAHE of numpy pics needs opencv-python (cv2), which is not installed") from e
            grid = (self.params["grid_size"],) * 2
            plane = (rgb2normspace(pic[:, :, :3])[:, :, 0] * 255).astype(np.uint8)
            chan = cv2.createCLAHE(clipLimit=self.params["clip_limit"], tileGridSize=grid).apply(plane).astype(np.float32) / 255.0
            acc.append(np.concatenate((pic, np.expand_dims(chan, axis=2)), axis=2))
        return acc


TRANSFORMS = {"match_histogram": MatchHistogram, "replace_histogram": ReplaceChannelWithHistogram, "gamma_equalize": GammaEqualize,
              "tospace": ToColorspace, "add_intensity_fromrgb": AddIntensityFromRgb, "add_clahe_fromrgb": AddClaheFromRgb}


def initialize_transforms(augmentations, mean_std):
    """``transform.initialize_transforms`` with the photometric names added: 'pil2np | match_histogram:eq | totensor | normalize' -> Compose"""
    registry = {**transform.TRANSFORMS, **TRANSFORMS}
    trans = []
    for aug in [x.strip() for x in augmentations.split("|") if x.strip()]:
        tname, *args = aug.split(":", 1)
        args = args[0].split(":") if args else []
        trans.append(registry[tname](*(list(mean_std) + args)) if "normalize" in aug else registry[tname](*args))
    return transform.Compose(trans)
