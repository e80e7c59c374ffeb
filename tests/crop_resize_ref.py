"""Float64 evaluation of the crop + bilinear resize + normalise that gdt_crop_resize_u8_batch and the host ``bilinear_resize`` compute in fp32, written
from the algorithm (cv2's INTER_LINEAR float path as ``cv2.resize(pic[y0:y0 + ch, x0:x0 + cw], (ow, oh))`` runs it on a float32 [0, 1] image):

    per axis, n_in = crop extent, n_out = output extent:  scale = n_in / (double) n_out
    output index d:  f = (float32)((d + 0.5) * scale - 0.5);  s = floor(f);  f -= s          (float32 subtraction)
                     s < 0: s = 0, f = 0;   s >= n_in - 1: s = n_in - 1, f = 0               (clamps to the crop box)
    taps s and min(s + 1, n_in - 1), weights (float32)(1.f - f) and f; horizontal blend, then vertical blend
    source values u8 / 255.f (float32); result (v - mean[c]) / std[c]

Only the coordinate, the weights and the source values are rounded to float32 (they are the reference's inputs to the blend); every product and sum
is exact in float64 here.  No loops over pixels: one table per axis."""
import numpy as np


def taps(n_in, n_out):
    """(first tap, second tap, float32 weight of the first, float32 weight of the second) per output index"""
    first, second, w0, w1 = [], [], [], []
    scale = float(n_in) / float(n_out)
    for d in range(n_out):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        f = np.float32(f - np.float32(s))
        if s < 0:
            s, f = 0, np.float32(0)
        if s >= n_in - 1:
            s, f = n_in - 1, np.float32(0)
        first.append(s)
        second.append(min(s + 1, n_in - 1))
        w0.append(np.float32(np.float32(1) - f))
        w1.append(f)
    return np.array(first), np.array(second), np.array(w0, dtype=np.float64), np.array(w1, dtype=np.float64)


def resize_unit(unit, out_w, out_h):
    """float H x W x C (values already what the blend reads) -> float64 out_h x out_w x C"""
    unit = np.asarray(unit, dtype=np.float64)
    x0, x1, a0, a1 = taps(unit.shape[1], out_w)
    y0, y1, b0, b1 = taps(unit.shape[0], out_h)
    rows = unit[:, x0] * a0[None, :, None] + unit[:, x1] * a1[None, :, None]
    return rows[y0] * b0[:, None, None] + rows[y1] * b1[:, None, None]


def crop_resize(u8, box, out_w, out_h, flip_src=False, flip_dst=False, mean=None, std=None):
    """uint8 H x W x 3, box (y0, x0, ch, cw) -> float64 3 x out_h x out_w"""
    y0, x0, ch, cw = box
    crop = u8[y0:y0 + ch, x0:x0 + cw]                                   # the reference slices first: nothing outside the box is read
    if flip_src:
        crop = crop[:, ::-1]
    unit = (crop.astype(np.float32) / np.float32(255)).astype(np.float64)
    out = resize_unit(unit, out_w, out_h)
    if flip_dst:
        out = out[:, ::-1]
    mean = np.zeros(3) if mean is None else np.asarray(mean, dtype=np.float32).astype(np.float64)
    std = np.ones(3) if std is None else np.asarray(std, dtype=np.float32).astype(np.float64)
    return np.ascontiguousarray(((out - mean) / std).transpose(2, 0, 1))


def gate(ref, std=None):
    """per element |got - ref| <= 4 * 2**-24 / std_c + 2**-22 * |ref|: three fp32 roundings of each blend on [0, 1] values, one each for the
    subtraction and the IEEE division"""
    std = np.ones(3) if std is None else np.asarray(std, dtype=np.float64)
    return 4 * 2.0 ** -24 / np.abs(std)[:, None, None] + 2.0 ** -22 * np.abs(ref)
