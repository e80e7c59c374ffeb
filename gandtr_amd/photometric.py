"""Photometric normalisation of the lightness channel on the device: histogram equalisation / matching and gamma equalisation.

Reference (per image, on the CPU through numpy, cv2 and scipy): ``channel_histogram_matching`` / ``channel2channel_histogram_matching`` /
``channel_gamma_matching`` and their ``image_*`` forms (mdir/components/data/transform/functional.py:96-133), ``rgb2normspace`` "lab" (:28-36).
Here a batch is processed by the HIP launches of gandtr_amd/csrc/photometric.hip; there is no CPU fallback.

The reference's named target histograms are data of the reference and are not part of this package: ``register_histogram`` / ``load_histograms`` make a
name known; ``"eq"`` (equalisation) needs none."""
import ctypes

import numpy as np
import torch

from . import _hip
from .clahe import _float3

HISTOGRAM_BINS = np.linspace(-0.00196078431372549, 1.0019607843137255, 257)       # functional.py:92
HISTOGRAM_CENTERS = np.linspace(0, 1, 256)                                        # functional.py:93
MODE_EQ, MODE_TARGET, MODE_PLANE = 0, 1, 2

_HISTOGRAMS = {}            # name -> float64 [256]
_device_cache = {}          # (device, name | "grid") -> float64 device tensor


def register_histogram(name, values):
    """Make ``name`` a target of ``match_channel`` / ``match_histogram``: ``values`` = its 256 bin masses (functional_consts.py HISTOGRAMS)."""
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    if values.shape != (256,):
        raise ValueError("a histogram has 256 bins, got %d" % values.size)
    if name == "eq":
        raise ValueError("'eq' is the equalisation target and cannot be registered")
    _HISTOGRAMS[name] = values
    for key in [k for k in _device_cache if k[1] == name]:
        del _device_cache[key]


def load_histograms(path):
    """``register_histogram`` for every array of an .npz file whose key starts with ``histogram_`` (the rest of the key is the name).  Returns the names."""
    names = []
    with np.load(path) as data:
        for key in data.files:
            if key.startswith("histogram_"):
                register_histogram(key[len("histogram_"):], data[key])
                names.append(key[len("histogram_"):])
    return names


def target_cdf(histogram):
    """(mode, float64 cdf [256] or None) of a target: "eq", a registered name or 256 bin masses.  HISTOGRAM_CDF of functional.py:94."""
    if isinstance(histogram, str):
        if histogram == "eq":
            return MODE_EQ, None
        return MODE_TARGET, np.cumsum(_HISTOGRAMS[histogram])             # KeyError for an unknown name, as HISTOGRAM_CDF[name]
    values = np.asarray(histogram, dtype=np.float64).reshape(-1)
    if values.shape != (256,):
        raise ValueError("a histogram has 256 bins, got %d" % values.size)
    return MODE_TARGET, np.cumsum(values)


def _grid(device):
    key = (str(device), "grid")
    if key not in _device_cache:
        _device_cache[key] = torch.from_numpy(np.concatenate([HISTOGRAM_BINS, HISTOGRAM_CENTERS])).to(device)
    return _device_cache[key]


def _device_cdf(histogram, device):
    mode, cdf = target_cdf(histogram)
    if mode == MODE_EQ:
        return mode, None
    if isinstance(histogram, str):                                        # the device copy of a registered cdf is cached per device
        key = (str(device), histogram)
        if key not in _device_cache:
            _device_cache[key] = torch.from_numpy(cdf).to(device)
        return mode, _device_cache[key]
    return mode, torch.from_numpy(cdf).to(device)


def _workspace(lib, n, h, w, device):
    need = ctypes.c_size_t()
    _hip.check(lib.gdt_photometric_workspace_bytes(n, h, w, ctypes.byref(need)))
    return torch.empty(need.value, dtype=torch.uint8, device=device)


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _images(x, who):
    if not x.is_cuda:
        raise ValueError("%s needs a tensor on a HIP device" % who)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("%s expects N x 3 x H x W, got %s" % (who, tuple(x.shape)))
    return x.detach().contiguous().float()


def _planes(chan, who):
    """fp32 planes [N][H][W] (or one [H][W]) on the device -> (contiguous [N][count] view source, squeeze)"""
    if not chan.is_cuda:
        raise ValueError("%s needs a tensor on a HIP device" % who)
    if chan.dim() not in (2, 3):
        raise ValueError("%s expects planes N x H x W or H x W, got %s" % (who, tuple(chan.shape)))
    squeeze = chan.dim() == 2
    return (chan[None] if squeeze else chan).detach().contiguous().float(), squeeze


def _pair(meanstd):
    return meanstd if meanstd is not None else (None, None)


def lightness(x, in_meanstd=None):
    """normalised lightness L / 100 of N x 3 x H x W RGB images: N x H x W (``rgb2normspace(img, "lab")[:, :, 0]``)"""
    lib = _hip.load()
    x = _images(x, "lightness")
    n, _, h, w = x.shape
    out = torch.empty((n, h, w), dtype=torch.float32, device=x.device)
    mean, std = _pair(in_meanstd)
    with torch.cuda.device(x.device):
        _hip.check(lib.gdt_lab_lightness_f32(x.data_ptr(), out.data_ptr(), n, h, w, _float3(std), _float3(mean), _stream(x)))
    return out


def to_lab(x, in_meanstd=None):
    """``rgb2normspace(img, "lab")`` of N x 3 x H x W RGB images: N x 3 x H x W planes (L / 100, (a + 128) / 255, (b + 128) / 255)"""
    lib = _hip.load()
    x = _images(x, "to_lab")
    n, _, h, w = x.shape
    out = torch.empty_like(x)
    mean, std = _pair(in_meanstd)
    with torch.cuda.device(x.device):
        _hip.check(lib.gdt_rgb2lab_f32(x.data_ptr(), out.data_ptr(), n, h, w, _float3(std), _float3(mean), _stream(x)))
    return out


def histogram256(chan):
    """``np.histogram(plane, HISTOGRAM_BINS)[0]`` of every plane: int64 N x 256 (or 256 for one H x W plane)"""
    lib = _hip.load()
    src, squeeze = _planes(chan, "histogram256")
    n, count = src.shape[0], src.shape[1] * src.shape[2]
    hist = torch.empty((n, 256), dtype=torch.int32, device=src.device)
    with torch.cuda.device(src.device):
        _hip.check(lib.gdt_hist256_f32(src.data_ptr(), n, count, _grid(src.device).data_ptr(), hist.data_ptr(), _stream(src)))
    hist = hist.long()
    return hist[0] if squeeze else hist


def _match_planes(src, mode, cdf, other):
    lib = _hip.load()
    n, count = src.shape[0], src.shape[1] * src.shape[2]
    out = torch.empty_like(src)
    count1 = other.shape[1] * other.shape[2] if other is not None else 0
    with torch.cuda.device(src.device):
        ws = _workspace(lib, n, 1, count, src.device)
        _hip.check(lib.gdt_match_channel_f32(src.data_ptr(), out.data_ptr(), n, count, mode, cdf.data_ptr() if cdf is not None else None,
                                             other.data_ptr() if other is not None else None, count1, _grid(src.device).data_ptr(),
                                             ws.data_ptr(), ws.numel(), _stream(src)))
    return out


def match_channel(chan, histogram):
    """``channel_histogram_matching(chan, histogram)`` on fp32 planes N x H x W (or H x W); ``histogram``: "eq", a registered name or 256 bin masses"""
    src, squeeze = _planes(chan, "match_channel")
    mode, cdf = _device_cdf(histogram, src.device)
    out = _match_planes(src, mode, cdf, None)
    return out[0] if squeeze else out


def match_channel_to(chan0, chan1):
    """``channel2channel_histogram_matching(chan0, chan1)``: plane i of ``chan0`` takes the histogram of plane i of ``chan1`` (whose size may differ)"""
    src, squeeze = _planes(chan0, "match_channel_to")
    other, _ = _planes(chan1, "match_channel_to")
    if other.shape[0] != src.shape[0] or other.device != src.device:
        raise ValueError("match_channel_to needs as many target planes as planes, on one device")
    out = _match_planes(src, MODE_PLANE, None, other)
    return out[0] if squeeze else out


def match_histogram(x, histogram, in_meanstd=None, out_meanstd=None):
    """``image_histogram_matching(img, histogram, "lab")`` on a batch of RGB images N x 3 x H x W (fp32, device); the affines as in ``clahe.clahe_lab``"""
    lib = _hip.load()
    x = _images(x, "match_histogram")
    mode, cdf = _device_cdf(histogram, x.device)
    n, _, h, w = x.shape
    y = torch.empty_like(x)
    in_mean, in_std = _pair(in_meanstd)
    out_mean, out_std = _pair(out_meanstd)
    with torch.cuda.device(x.device):
        ws = _workspace(lib, n, h, w, x.device)
        _hip.check(lib.gdt_match_histogram_lab_f32(x.data_ptr(), y.data_ptr(), n, h, w, _float3(in_std), _float3(in_mean), _float3(out_mean),
                                                   _float3(out_std), mode, cdf.data_ptr() if cdf is not None else None,
                                                   _grid(x.device).data_ptr(), ws.data_ptr(), ws.numel(), _stream(x)))
    return y


def gamma_channel(chan, target, return_gamma=False, return_evaluations=False):
    """``channel_gamma_matching(chan, target)`` on fp32 planes N x H x W (or H x W): plane ** gamma with mean(plane ** gamma) = target, gamma found per
    plane on the device.  ``return_gamma``: also the float64 gammas [N] (device); ``return_evaluations``: also the function evaluations of each solve."""
    lib = _hip.load()
    src, squeeze = _planes(chan, "gamma_channel")
    n, count = src.shape[0], src.shape[1] * src.shape[2]
    out = torch.empty_like(src)
    gamma = torch.empty(n, dtype=torch.float64, device=src.device)
    evals = torch.empty(n, dtype=torch.int32, device=src.device)
    with torch.cuda.device(src.device):
        _hip.check(lib.gdt_gamma_channel_f32(src.data_ptr(), out.data_ptr(), n, count, float(target), gamma.data_ptr(), evals.data_ptr(), _stream(src)))
    res = (out[0] if squeeze else out,) + ((gamma,) if return_gamma else ()) + ((evals,) if return_evaluations else ())
    return res[0] if len(res) == 1 else res


def gamma_equalize(x, target, in_meanstd=None, out_meanstd=None, return_gamma=False, return_evaluations=False):
    """``image_gamma_matching(img, target, "lab")`` on a batch of RGB images N x 3 x H x W (fp32, device); the affines as in ``clahe.clahe_lab``"""
    lib = _hip.load()
    x = _images(x, "gamma_equalize")
    n, _, h, w = x.shape
    y = torch.empty_like(x)
    gamma = torch.empty(n, dtype=torch.float64, device=x.device)
    evals = torch.empty(n, dtype=torch.int32, device=x.device)
    in_mean, in_std = _pair(in_meanstd)
    out_mean, out_std = _pair(out_meanstd)
    with torch.cuda.device(x.device):
        ws = _workspace(lib, n, h, w, x.device)
        _hip.check(lib.gdt_gamma_equalize_lab_f32(x.data_ptr(), y.data_ptr(), n, h, w, _float3(in_std), _float3(in_mean), _float3(out_mean),
                                                  _float3(out_std), float(target), gamma.data_ptr(), evals.data_ptr(), ws.data_ptr(), ws.numel(),
                                                  _stream(x)))
    res = (y,) + ((gamma,) if return_gamma else ()) + ((evals,) if return_evaluations else ())
    return res[0] if len(res) == 1 else res
