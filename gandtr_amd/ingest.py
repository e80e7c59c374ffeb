"""Image ingest on the device after decoding.

Reference (per image, on the CPU through Pillow / numpy): ``imresize`` = ``img.thumbnail((s, s), LANCZOS)``
(mdir/external/cirtorch/datasets/datahelpers.py:75-82, called from genericdataset.py:66-102) followed by the hub transform
``pil2np | apply_clahe:1.0 | totensor | normalize`` (mdir/hub/embedding.yml:14, core_transforms.py:35-100).
Here the decoded uint8 H x W x 3 image is uploaded once; resize (bit-identical to Pillow), [0, 1] scaling, optional CLAHE and
normalisation run as HIP launches (gandtr_amd/csrc/ingest.hip, clahe.hip).  The size / reducing-gap plan below mirrors Pillow's
Python layer (PIL/Image.py: thumbnail, resize); JPEG decoding stays on the host.  No CPU fallback."""
import collections
import ctypes
import math
import random

import torch

from . import _hip
from .components.data import transform as host


def thumbnail_size(width, height, imsize):
    """size Image.thumbnail((imsize, imsize)) resizes to, or None when the image already fits (PIL/Image.py preserve_aspect_ratio)"""
    x = y = math.floor(imsize)
    if x >= width and y >= height:
        return None

    def round_aspect(number, key):
        return max(min(math.floor(number), math.ceil(number), key=key), 1)

    aspect = width / height
    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    return x, y


def reduce_plan(width, height, out_w, out_h, reducing_gap=2.0):
    """Image.resize(..., reducing_gap): integer box-reduction factors and the source box of the resampling step (in pixels of the
    reduced image).  thumbnail passes the full image as the box, for which Pillow's safe box is the full image as well."""
    fx = int(width / out_w / reducing_gap) or 1
    fy = int(height / out_h / reducing_gap) or 1
    if fx > 1 or fy > 1:
        return fx, fy, (0.0, 0.0, width / fx, height / fy)
    return 1, 1, (0.0, 0.0, float(width), float(height))


def _f(vals, n):
    if vals is None:
        return None
    vals = [float(v) for v in vals]
    if len(vals) != n:
        raise ValueError("expected %d per-channel values, got %d" % (n, len(vals)))
    return (ctypes.c_float * n)(*vals)


def resize(img, out_w, out_h, factors=(1, 1), box=None, want_u8=True, mean_std=None, want_chw=False):
    """Pillow's reduce(factors) + resize((out_w, out_h), LANCZOS, box) on a uint8 H x W x C device tensor.
    Returns (uint8 out_h x out_w x C or None, fp32 C x out_h x out_w or None)."""
    lib = _hip.load()
    if not img.is_cuda or img.dtype != torch.uint8 or img.dim() != 3:
        raise ValueError("ingest needs a uint8 H x W x C tensor on a HIP device")
    img = img.contiguous()
    h, w, c = img.shape
    fx, fy = factors
    dst = torch.empty((out_h, out_w, c), dtype=torch.uint8, device=img.device) if want_u8 else None
    chw = torch.empty((c, out_h, out_w), dtype=torch.float32, device=img.device) if want_chw else None
    mean, std = mean_std if mean_std is not None else (None, None)
    need = ctypes.c_size_t()
    with torch.cuda.device(img.device):
        _hip.check(lib.gdt_ingest_workspace_bytes(h, w, c, fx, fy, out_w, out_h, ctypes.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=img.device)
        _hip.check(lib.gdt_ingest_resize_u8(img.data_ptr(), h, w, c, fx, fy, _f(box, 4), out_w, out_h,
                                            dst.data_ptr() if want_u8 else None, chw.data_ptr() if want_chw else None,
                                            _f(mean, c), _f(std, c), ws.data_ptr(), ws.numel(),
                                            torch.cuda.current_stream(img.device).cuda_stream))
    return dst, chw


def _plan(img, imsize):
    h, w, _ = img.shape
    size = thumbnail_size(w, h, imsize) if imsize is not None else None
    if size is None:
        size = (w, h)
    fx, fy, box = reduce_plan(w, h, size[0], size[1]) if size != (w, h) else (1, 1, None)
    return size, (fx, fy), box


def imresize(img, imsize):
    """datahelpers.imresize: ``img.thumbnail((imsize, imsize), LANCZOS)`` on a decoded uint8 H x W x C device tensor."""
    size, factors, box = _plan(img, imsize)
    if size == (img.shape[1], img.shape[0]):
        return img
    return resize(img, size[0], size[1], factors, box)[0]


def ingest(img, imsize, mean, std, clahe_clip=None, clahe_grid=8):
    """decoded uint8 H x W x 3 (device) -> fp32 3 x h x w, what ``imresize`` followed by
    ``pil2np | [apply_clahe:clip] | totensor | normalize`` produce (hub transform: mdir/hub/embedding.yml:14)."""
    size, factors, box = _plan(img, imsize)
    if clahe_clip is None:
        return resize(img, size[0], size[1], factors, box, want_u8=False, mean_std=(mean, std), want_chw=True)[1]
    from . import clahe
    unit = resize(img, size[0], size[1], factors, box, want_u8=False, want_chw=True)[1]          # [0, 1] RGB planes
    return clahe.clahe_lab(unit[None], clahe_clip, clahe_grid, None, (mean, std))[0]


def resize_many(images, plans, want_u8=True, mean_std=None, want_chw=False):
    """``resize`` for a list of uint8 H x W x C device tensors of different sizes in ONE library call (gdt_ingest_resize_u8_batch: three
    launches for the whole list when the images are RGB).  ``plans``: per image ``((out_w, out_h), (fx, fy), box or None)``.
    Returns (list of uint8 outputs or None, list of fp32 C x h x w outputs or None)."""
    lib = _hip.load()
    if not images:
        return ([] if want_u8 else None), ([] if want_chw else None)
    dev, c = images[0].device, images[0].shape[2]
    images = [img.contiguous() for img in images]
    for img in images:
        if not img.is_cuda or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != c or img.device != dev:
            raise ValueError("ingest needs uint8 H x W x C tensors with the same channel count on one HIP device")
    n = len(images)
    items = (_hip.IngestItem * n)()
    u8 = [None] * n
    chw = [None] * n
    # one allocation per output kind for the whole list (views of 16-byte aligned slices): 64 small allocations cost more than the kernels
    counts = [c * size[0] * size[1] for size, _, _ in plans]
    starts = [0] * n
    for i in range(1, n):
        starts[i] = starts[i - 1] + (counts[i - 1] + 15) // 16 * 16
    total = starts[-1] + counts[-1]
    flat_u8 = torch.empty(total, dtype=torch.uint8, device=dev) if want_u8 else None
    flat_f = torch.empty(total, dtype=torch.float32, device=dev) if want_chw else None
    for i, (img, (size, factors, box)) in enumerate(zip(images, plans)):
        it = items[i]
        it.src, it.h, it.w = img.data_ptr(), img.shape[0], img.shape[1]
        it.fx, it.fy = factors
        if box is not None:
            it.box = (ctypes.c_float * 4)(*[float(v) for v in box])
        it.out_w, it.out_h = size
        if want_u8:
            u8[i] = flat_u8[starts[i]:starts[i] + counts[i]].view(size[1], size[0], c)
            it.dst_hwc = u8[i].data_ptr()
        if want_chw:
            chw[i] = flat_f[starts[i]:starts[i] + counts[i]].view(c, size[1], size[0])
            it.dst_chw = chw[i].data_ptr()
    mean, std = mean_std if mean_std is not None else (None, None)
    need = ctypes.c_size_t()
    with torch.cuda.device(dev):
        _hip.check(lib.gdt_ingest_batch_workspace_bytes(items, n, c, ctypes.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        _hip.check(lib.gdt_ingest_resize_u8_batch(items, n, c, _f(mean, c), _f(std, c), ws.data_ptr(), ws.numel(),
                                                  torch.cuda.current_stream(dev).cuda_stream))
    return (u8 if want_u8 else None), (chw if want_chw else None)


def ingest_many(images, imsize, mean, std, clahe_clip=None, clahe_grid=8, streams=4):
    """``ingest`` over a list of decoded images of different sizes (the reference is batch-1 for exactly that reason,
    imageretrievalnet.py:319-322): the resampling of the whole list is one library call / three launches (``resize_many``); only the
    optional CLAHE still runs per image (its tile grid depends on the image size).  ``streams`` is kept for callers of the earlier
    per-image form and ignored.  Returns a list of fp32 3 x h x w tensors in input order."""
    if not images:
        return []
    sizes = list(imsize) if isinstance(imsize, (list, tuple)) else [imsize] * len(images)      # (per image: the dataset scales cropped queries, genericdataset.py:89-91)
    plans = [_plan(img, s) for img, s in zip(images, sizes)]
    if clahe_clip is None:
        return resize_many(images, plans, want_u8=False, mean_std=(mean, std), want_chw=True)[1]
    from . import clahe
    unit = resize_many(images, plans, want_u8=False, want_chw=True)[1]                              # [0, 1] RGB planes
    return [clahe.clahe_lab(u[None], clahe_clip, clahe_grid, None, (mean, std))[0] for u in unit]


def crop_resize(images, boxes, out_w, out_h, flips=None, mean_std=None, out=None):
    """``cv2.resize(pic[y0:y0 + ch, x0:x0 + cw], (out_w, out_h))`` + ``totensor | normalize`` for a list of decoded uint8 H x W x 3 device tensors of
    different sizes in ONE launch (gdt_crop_resize_u8_batch, gandtr_amd/csrc/crop_resize.hip).  ``boxes``: per image ``(y0, x0, ch, cw)``; ``flips``:
    per image ``(flip_src, flip_dst)`` -- mirror the box before / the output after the resample; ``mean_std`` None = the unit image.  A box of the
    output's size is a crop + convert, bit-identical to ``((u8 / 255) - mean) / std``.  ``out``: an fp32 N x 3 x out_h x out_w tensor or a list of N
    contiguous fp32 3 x out_h x out_w views (slices of several tensors: the call takes one destination per image); default a new tensor.  Returns it."""
    lib = _hip.load()
    n = len(images)
    if n == 0:
        raise ValueError("crop_resize needs at least one image")
    dev = images[0].device
    images = [img.contiguous() for img in images]
    for img in images:
        if not img.is_cuda or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or img.device != dev:
            raise ValueError("crop_resize needs uint8 H x W x 3 tensors on one HIP device")
    if out is None:
        out = torch.empty((n, 3, out_h, out_w), dtype=torch.float32, device=dev)
    dsts = list(out)                                                     # (a tensor's rows, or the caller's list of views)
    if len(dsts) != n or any(d.shape != (3, out_h, out_w) or d.dtype != torch.float32 or d.device != dev or not d.is_contiguous() for d in dsts):
        raise ValueError("crop_resize: out must be %d contiguous fp32 3 x %d x %d tensors on the images' device" % (n, out_h, out_w))
    items = (_hip.CropItem * n)()
    for i, (img, (y0, x0, ch, cw)) in enumerate(zip(images, boxes)):
        it = items[i]
        it.src, it.h, it.w = img.data_ptr(), img.shape[0], img.shape[1]
        it.x0, it.y0, it.cw, it.ch = int(x0), int(y0), int(cw), int(ch)
        if flips is not None:
            it.flip_src, it.flip_dst = int(bool(flips[i][0])), int(bool(flips[i][1]))
        it.dst_chw = dsts[i].data_ptr()
    mean, std = mean_std if mean_std is not None else (None, None)
    need = ctypes.c_size_t()
    with torch.cuda.device(dev):
        _hip.check(lib.gdt_crop_resize_workspace_bytes(n, out_w, out_h, ctypes.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        _hip.check(lib.gdt_crop_resize_u8_batch(items, n, out_w, out_h, _f(mean, 3), _f(std, 3), ws.data_ptr(), ws.numel(),
                                                torch.cuda.current_stream(dev).cuda_stream))
    return out


Geometry = collections.namedtuple("Geometry", "box flip_src resample flip_dst out")
Geometry.__doc__ = """What a chain's geometric steps do to one pic: the source ``box`` (y0, x0, ch, cw) in the decoded image, ``flip_src`` (mirror the box),
``resample`` -- ("none",), ("bilinear", ow, oh) or ("lanczos", n) (Pillow's thumbnail to n) --, ``flip_dst`` (mirror the result), ``out`` = (h, w) of it."""

_RESAMPLERS = ("scalecrop", "centerscalecrop", "downscale")
_CROPS = ("center_crop", "square_crop")


class DeviceTransform:
    """Device-side counterpart of the ``.transform`` the hub attaches to a network (mdir/hub/model.py:38-42 builds it from
    ``runtime.data.transforms``, e.g. ``pil2np | apply_clahe:1.0 | totensor | normalize``) and of the ``transforms:`` chain of a dataset
    (mdir/components/data/dataset/__init__.py:35-41, e.g. ``pil2np | scalecrop:256_256:0.8_1 | totensor | normalize``): takes DECODED images as uint8
    H x W x 3 tensors on the device and returns the fp32 3 x h x w tensors the network expects.  Supported steps: pil2np, apply_clahe[:clip[:grid[:lab]]],
    totensor, normalize and the geometric steps scalecrop:W_H[:lo_hi], centerscalecrop:W_H[:s], downscale:N, center_crop:W_H, square_crop, mirror[:p]
    (augmentation_transforms.py:24-164) in the chain shape ``crops / mirrors, at most one resampling step, mirrors``; apply_clahe comes after them.
    With ``photometric=True`` a chain may hold, in apply_clahe's place, ONE of ``match_histogram:NAME[:lab]`` or ``gamma_equalize:T[:lab]``
    (photometric_transforms.py:56-104; gandtr_amd/photometric.py); without it those names raise KeyError like every unknown step.

    ``__call__(img, imsize=None)`` serves chains without geometric steps (the hub's).  A chain with them runs as ``plan`` (host, draws the random numbers
    the reference draws) + ``apply_many`` (device, one crop-resize launch for a whole batch)."""

    def __init__(self, augmentations, mean_std, photometric=False):
        self.mean, self.std = [float(v) for v in mean_std[0]], [float(v) for v in mean_std[1]]
        self.clahe_clip, self.clahe_grid, self.normalize = None, 8, False
        self.photometric = None                                            # ("match_histogram", name) or ("gamma_equalize", target), with photometric=True
        self.spec = augmentations
        self.geometric = []                                                # (name, host transform): the one statement of each step's geometry
        resampled = False
        for step in [t.strip() for t in augmentations.split("|") if t.strip()]:
            name, *args = step.split(":")
            if name in ("pil2np", "totensor"):
                continue
            if name == "normalize":
                self.normalize = True
            elif name == "apply_clahe":
                if self.photometric is not None:
                    raise NotImplementedError("one of apply_clahe, match_histogram, gamma_equalize per chain on the HIP path: '%s'" % augmentations)
                self.clahe_clip = float(args[0]) if args else 4.0          # ApplyClahe defaults (photometric_transforms.py:31)
                self.clahe_grid = int(args[1]) if len(args) > 1 else 8
                if len(args) > 2 and args[2].lower() != "lab":
                    raise NotImplementedError("Colorspace %s is not supported on the HIP path" % args[2])
            elif photometric and name in ("match_histogram", "gamma_equalize"):
                # (photometric_transforms.py:56-104) one of them, in the position apply_clahe may take; it normalises the result itself
                if self.photometric is not None or self.clahe_clip is not None:
                    raise NotImplementedError("one of apply_clahe, match_histogram, gamma_equalize per chain on the HIP path: '%s'" % augmentations)
                if not args:
                    raise TypeError("%s needs its %s" % (name, "histogram" if name == "match_histogram" else "target"))
                if len(args) > 1 and args[1].lower() != "lab":
                    raise NotImplementedError("Colorspace %s is not supported on the HIP path" % args[1])
                if name == "gamma_equalize":
                    target = float(args[0])
                    assert target > 0 and target < 1, target
                    self.photometric = (name, target)
                else:
                    self.photometric = (name, args[0])
            elif name in _RESAMPLERS + _CROPS + ("mirror",):
                if self.clahe_clip is not None:
                    raise NotImplementedError("apply_clahe before a geometric step is not supported on the HIP path: '%s'" % augmentations)
                if self.photometric is not None:
                    raise NotImplementedError("%s before a geometric step is not supported on the HIP path: '%s'" % (self.photometric[0], augmentations))
                if resampled and name != "mirror":
                    raise NotImplementedError("only mirrors may follow a resampling step on the HIP path: '%s'" % augmentations)
                resampled = resampled or name in _RESAMPLERS
                self.geometric.append((name, host.TRANSFORMS[name](*args)))
            else:
                raise KeyError("transform '%s' has no device implementation" % name)

    def _mean_std(self):
        return (self.mean, self.std) if self.normalize else ([0.0] * 3, [1.0] * 3)

    def __call__(self, img, imsize=None):
        if self.geometric:
            raise NotImplementedError("a chain with geometric steps runs through plan() + apply_many(): '%s'" % self.spec)
        mean, std = self._mean_std()
        if self.photometric is not None:
            return self._photometric(ingest(img, imsize, [0.0] * 3, [1.0] * 3)[None])[0]
        return ingest(img, imsize, mean, std, self.clahe_clip, self.clahe_grid)

    def _photometric(self, unit):
        """the chain's match_histogram / gamma_equalize step on a batch of unit images N x 3 x h x w, normalised on the way out"""
        from . import photometric
        kind, arg = self.photometric
        if kind == "match_histogram":
            return photometric.match_histogram(unit, arg, None, self._mean_std())
        return photometric.gamma_equalize(unit, arg, None, self._mean_std())

    def plan(self, shapes, rng=random):
        """One ``Geometry`` per pic of ONE item (``shapes``: their decoded (h, w)).  Pure host code; draws from ``rng`` exactly what the reference's
        transforms draw on the same pics, in their order, so ``random.seed(s)`` reproduces its crops and flips."""
        state = [dict(box=(0, 0, int(h), int(w)), flip_src=False, resample=("none",), flip_dst=False, out=(int(h), int(w))) for h, w in shapes]
        for _, step in self.geometric:
            for st, op in zip(state, step.ops([st["out"] for st in state], rng)):
                if op is None:
                    continue
                if op[0] == "flip":
                    key = "flip_src" if st["resample"] == ("none",) else "flip_dst"
                    st[key] = not st[key]
                    continue
                assert st["resample"] == ("none",), self.spec               # (the constructor refused such a chain)
                if op[0] == "lanczos":
                    size = thumbnail_size(st["out"][1], st["out"][0], op[1])
                    if size is not None:
                        st["resample"], st["out"] = ("lanczos", op[1]), (size[1], size[0])
                    continue
                y0, x0, ch, cw = op[1:5]
                by, bx, _, bw = st["box"]
                st["box"] = (by + y0, bx + (bw - x0 - cw if st["flip_src"] else x0), ch, cw)       # (a crop of the mirrored box, in unmirrored columns)
                st["out"] = (ch, cw)
                if op[0] == "bilinear":
                    st["resample"], st["out"] = ("bilinear", op[5], op[6]), (op[6], op[5])
        return [Geometry(**st) for st in state]

    def apply_many(self, decoded_items, plans):
        """``decoded_items``: per item its pics as decoded uint8 H x W x 3 device tensors; ``plans``: per item what ``plan`` returned for it.  Returns the
        collated batch: one fp32 N x 3 x h x w tensor per column.  Every pic without a LANCZOS step goes through ONE gdt_crop_resize_u8_batch launch
        per distinct output size (one for the whole batch when the columns agree, as in every published scenario); LANCZOS pics go through
        ``resize_many`` on the cropped view (Pillow's integer arithmetic: the reference's ``(pic * 255).astype(uint8)`` round trip is the identity
        on decoded 8-bit data).  Items that end with different sizes raise RuntimeError, as ``default_collate`` does."""
        n, ncols = len(decoded_items), len(decoded_items[0])
        dev = decoded_items[0][0].device
        own_norm = self.clahe_clip is not None or self.photometric is not None
        mean_std = None if own_norm else self._mean_std()                        # (CLAHE and the photometric steps take the unit image and normalise themselves)
        columns = []
        for c in range(ncols):
            sizes = [plans[i][c].out for i in range(n)]
            if any(s != sizes[0] for s in sizes):
                raise RuntimeError("stack expects each tensor to be equal size, but got %s at entry 0 and %s at entry %d" % (
                    [3, *sizes[0]], [3, *next(s for s in sizes if s != sizes[0])], next(i for i, s in enumerate(sizes) if s != sizes[0])))
            columns.append(torch.empty((n, 3, sizes[0][0], sizes[0][1]), dtype=torch.float32, device=dev))
        direct, lanczos = {}, []
        for i in range(n):
            for c in range(ncols):
                g = plans[i][c]
                (lanczos if g.resample[0] == "lanczos" else direct.setdefault(g.out, [])).append((i, c))
        for (oh, ow), where in direct.items():                              # straight into the columns: one destination view per pic
            crop_resize([decoded_items[i][c] for i, c in where], [plans[i][c].box for i, c in where], ow, oh,
                        [(plans[i][c].flip_src, plans[i][c].flip_dst) for i, c in where], mean_std, [columns[c][i] for i, c in where])
        if lanczos:
            views = []
            for i, c in lanczos:
                g = plans[i][c]
                y0, x0, ch, cw = g.box
                view = decoded_items[i][c][y0:y0 + ch, x0:x0 + cw]
                views.append((view.flip(1) if g.flip_src else view).contiguous())
            outs = resize_many(views, [_plan(v, plans[i][c].resample[1]) for v, (i, c) in zip(views, lanczos)], want_u8=False, mean_std=mean_std,
                               want_chw=True)[1]
            for o, (i, c) in zip(outs, lanczos):
                columns[c][i].copy_(o.flip(2) if plans[i][c].flip_dst else o)
        if self.clahe_clip is not None:
            from . import clahe
            columns = [clahe.clahe_lab(col, self.clahe_clip, self.clahe_grid, None, self._mean_std()) for col in columns]
        if self.photometric is not None:
            columns = [self._photometric(col) for col in columns]
        return columns

    def __repr__(self):
        return "%s(%s, mean=%s, std=%s)" % (type(self).__name__, self.spec, self.mean, self.std)
