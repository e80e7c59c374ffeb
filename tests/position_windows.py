"""Batches whose images hold the SAME content at different places, and the output windows that must then be equal bit for bit.

A conv's output pixel is a function of its input neighbourhood and the weights.  A patch kernel computes it in a 16 x 16 tile of a
persistent workgroup's list, from a halo staged in pieces -- none of which may show in the value.  Three families of batches say so:

  zero_canvas     image k holds the content A at offset (dy_k, dx_k) in a canvas of zeros (zero padding and zero canvas are the same numbers,
                  so a window may touch the canvas border of a zero-padded conv);
  reflect_border  A in a canvas corner, where the layer's own reflect padding acts, against the host-side reflect extension of A in the
                  canvas interior;
  roll_family     image k is torch.roll of image 0 (full images: this is the family that keeps InstanceNorm statistics unchanged).

Each returns the batch and a list of Pair: out[img, :, y:y+h, x:x+w] must equal out[ref, :, ry:ry+h, rx:rx+w].  compare() checks them with
torch.equal and, on a mismatch, says WHERE in the 16 x 16 patch and in which output channels (mod 64) the differing outputs lie."""
import collections

import torch
import torch.nn.functional as F

PATCH = 16

Pair = collections.namedtuple("Pair", "img y x ref ry rx h w")
Conv = collections.namedtuple("Conv", "k stride pad transposed opad")

S1 = Conv(3, 1, 1, False, 0)          # Conv2d(k3, s1, p1)
S2 = Conv(3, 2, 1, False, 0)          # Conv2d(k3, s2, p1)
T2 = Conv(3, 2, 1, True, 1)           # ConvTranspose2d(k3, s2, p1, op1)
S1K7 = Conv(7, 1, 3, False, 0)        # Conv2d(k7, s1, p3)
S2K7 = Conv(7, 2, 3, False, 0)        # Conv2d(k7, s2, p3)
S1K4 = Conv(4, 1, 1, False, 0)        # Conv2d(k4, s1, p1): the output is one smaller than the input
S2K4 = Conv(4, 2, 1, False, 0)        # Conv2d(k4, s2, p1)
T4 = Conv(4, 2, 1, True, 0)           # ConvTranspose2d(k4, s2, p1)


def out_size(conv, n):
    """output extent of an input extent n"""
    if conv.transposed:
        return (n - 1) * conv.stride - 2 * conv.pad + conv.k + conv.opad
    return (n + 2 * conv.pad - conv.k) // conv.stride + 1


def window(conv, d, n):
    """(start, length) of the output window of content [d, d + n) along one axis.  Forward convs: the outputs a canvas of the content's own
    size would have, i. e. for an odd kernel those CENTRED on a content pixel (n at stride 1, n - 1 for the 4 x 4 kernel; stride 2: even
    offsets only, every second one).  Transposed: the 2n outputs of the n content pixels' own sub-pixel cells"""
    if conv.transposed:
        return conv.stride * d, conv.stride * n
    if d % conv.stride:
        raise ValueError("offset %d is no multiple of the stride %d" % (d, conv.stride))
    if conv.stride == 1:
        return d, n + 2 * conv.pad - conv.k + 1
    return d // conv.stride, (n + conv.stride - 1) // conv.stride


def touched(conv, d, n):
    """(start, length) of ALL outputs that read a content pixel of [d, d + n), not clipped to the canvas: the window and a margin around it"""
    if conv.transposed:                               # input i feeds outputs s i - p .. s i - p + k - 1
        lo, hi = conv.stride * d - conv.pad, conv.stride * (d + n - 1) - conv.pad + conv.k - 1
    else:                                             # output o reads inputs s o - p .. s o - p + k - 1
        lo, hi = -((conv.k - 1 - conv.pad - d) // conv.stride), (d + n - 1 + conv.pad) // conv.stride
    return lo, hi - lo + 1


def zero_canvas(content, canvas, offsets, conv=S1):
    """content [C][h][w] (h, w odd, no multiples of 16) at offsets[k] in image k of a zero batch [len(offsets)][C][H][W]; image k's window
    against image 0's"""
    c, h, w = content.shape
    hh, ww = canvas
    if not (h % 2 and w % 2 and h % PATCH and w % PATCH):
        raise ValueError("content %d x %d: both sizes odd and no multiple of %d" % (h, w, PATCH))
    batch = torch.zeros(len(offsets), c, hh, ww, dtype=content.dtype)
    wins = []
    for k, (dy, dx) in enumerate(offsets):
        if not (0 <= dy <= hh - h and 0 <= dx <= ww - w):
            raise ValueError("offset (%d, %d): the content leaves the canvas" % (dy, dx))
        batch[k, :, dy:dy + h, dx:dx + w] = content
        (y, oh), (x, ow) = window(conv, dy, h), window(conv, dx, w)
        if y + oh > out_size(conv, hh) or x + ow > out_size(conv, ww):
            raise ValueError("offset (%d, %d): the window leaves the output" % (dy, dx))
        wins.append((y, x, oh, ow))
    pairs = [Pair(k, y, x, 0, wins[0][0], wins[0][1], oh, ow) for k, (y, x, oh, ow) in enumerate(wins) if k]
    return batch, pairs


def reflect_border(content, canvas, depth, tl_offsets, br_offsets):
    """stride-1 conv with reflect padding `depth` (= k // 2).  Image 0: content in the top-left canvas corner; image 1: in the bottom-right
    corner.  Then one image per entry of tl_offsets: the content reflect-extended by `depth` rows above and columns to the left, at that
    offset; and per entry of br_offsets: extended below and to the right.  Every output of the content in a corner image -- its border rows
    and columns included -- is paired with the output in the interior image that sees the same k x k input pixels (beyond the other two
    sides of the content both see zeros).  The inner part of the content, `depth` away from its border, links the two corner images."""
    c, h, w = content.shape
    hh, ww = canvas
    p = depth
    ext_tl = F.pad(content[None], (p, 0, p, 0), mode="reflect")[0]
    ext_br = F.pad(content[None], (0, p, 0, p), mode="reflect")[0]
    batch = torch.zeros(2 + len(tl_offsets) + len(br_offsets), c, hh, ww, dtype=content.dtype)
    if h + p > hh or w + p > ww:
        raise ValueError("the content and %d zeros beyond it do not fit the canvas" % p)
    batch[0, :, :h, :w] = content
    batch[1, :, hh - h:, ww - w:] = content
    pairs = [Pair(1, hh - h + p, ww - w + p, 0, p, p, h - 2 * p, w - 2 * p)]
    k = 2
    for oy, ox in tl_offsets:                           # the content's body at (oy + p, ox + p); zeros for `depth` beyond its lower and right side
        if not (0 <= oy and oy + p + h + p <= hh and 0 <= ox and ox + p + w + p <= ww):
            raise ValueError("top-left extension at (%d, %d) leaves the canvas interior" % (oy, ox))
        batch[k, :, oy:oy + h + p, ox:ox + w + p] = ext_tl
        pairs.append(Pair(k, oy + p, ox + p, 0, 0, 0, h, w))
        k += 1
    for oy, ox in br_offsets:                           # the body at (oy, ox); zeros for `depth` beyond its upper and left side
        if not (p <= oy and oy + h + p <= hh and p <= ox and ox + w + p <= ww):
            raise ValueError("bottom-right extension at (%d, %d) leaves the canvas interior" % (oy, ox))
        batch[k, :, oy:oy + h + p, ox:ox + w + p] = ext_br
        pairs.append(Pair(k, oy, ox, 1, hh - h, ww - w, h, w))
        k += 1
    return batch, pairs


def _roll_segments(n, d, p):
    """along one axis of extent n rolled by d: (start in the rolled image, start in image 0, length) of the outputs whose neighbourhood of
    depth p crosses neither image's border nor the wrap seam"""
    d %= n
    segs = [(d + p, p, n - 2 * p - d), (p, n - d + p, d - 2 * p)] if d else [(p, p, n - 2 * p)]
    return [s for s in segs if s[2] > 0]


def roll_family(image, shifts, depth=1):
    """image [C][H][W]; image k of the batch is torch.roll(image, shifts[k]) (shifts[0] must be (0, 0)).  Stride-1 layers of padding
    `depth`; depth 0: a pointwise op, every output of the rolled image pairs with one of image 0"""
    if tuple(shifts[0]) != (0, 0):
        raise ValueError("image 0 is the unrolled one")
    c, hh, ww = image.shape
    batch = torch.stack([torch.roll(image, (dy, dx), (1, 2)) for dy, dx in shifts])
    pairs = []
    for k, (dy, dx) in enumerate(shifts):
        if k:
            pairs += [Pair(k, y, x, 0, ry, rx, h, w) for y, ry, h in _roll_segments(hh, dy, depth) for x, rx, w in _roll_segments(ww, dx, depth)]
    return batch, pairs


# ---- the placements the device tests run (tests/test_hip_translation_exact.py); tests/test_position_windows_cpu.py holds each to the coverage conditions

_O8 = [(0, 0), (43, 45), (15, 1), (1, 15), (16, 17), (33, 31), (27, 40), (40, 8)]
_O16 = _O8 + [(5, 22), (22, 5), (8, 37), (37, 12), (12, 44), (43, 0), (0, 45), (30, 26)]
_TL = [(14, 0), (15, 14), (0, 15), (30, 31), (41, 43), (20, 9), (8, 27)]              # extension origins: the content's body one further
_BR = [(1, 1), (15, 16), (16, 15), (42, 44), (31, 33), (10, 25), (26, 7)]
_ROLL = [(0, 0), (1, 15), (15, 1), (16, 17), (5, 22), (22, 5), (35, 29), (8, 40), (40, 8), (47, 48), (63, 63), (31, 33), (12, 44), (27, 2), (2, 27), (50, 19)]

PLACEMENTS = {
    # 64 x 64 canvases, content 21 x 19: every window spans a patch seam in both directions
    "zero64_n16": dict(family="zero", conv=S1, canvas=(64, 64), content=(21, 19), offsets=_O16),
    "zero64_n8": dict(family="zero", conv=S1, canvas=(64, 64), content=(21, 19), offsets=_O8),
    # ragged 76 x 92 (patch rows 64 .. 75 and columns 80 .. 91 are partial)
    "zero_ragged": dict(family="zero", conv=S1, canvas=(76, 92), content=(21, 19),
                        offsets=[(0, 0), (55, 73), (15, 1), (1, 15), (47, 65), (33, 70), (50, 40), (20, 61)]),
    # stride 2: input 128 x 128, content 37 x 41 -> windows 19 x 21 of the 64 x 64 output, at _O8
    "zero_s2": dict(family="zero", conv=S2, canvas=(128, 128), content=(37, 41), offsets=[(2 * y, 2 * x) for y, x in _O8[:1] + [(45, 43)] + _O8[2:]]),
    # transposed: input 64 x 64, content 11 x 13 -> windows 22 x 26 of the 128 x 128 output
    "zero_t2": dict(family="zero", conv=T2, canvas=(64, 64), content=(11, 13), offsets=_O8[:1] + [(53, 51)] + _O8[2:]),
    # a REFLECT layer on a zero canvas (the epilogue-residual layer): the content stays one pixel off the canvas border, where the layer's
    # padding would mirror it
    "zero64_inner": dict(family="zero", conv=S1, canvas=(64, 64), content=(21, 19), offsets=[(1, 1), (42, 44), (15, 2), (2, 15), (16, 17), (33, 31), (27, 29), (40, 8)], inner=True),
    "reflect64_n16": dict(family="reflect", conv=S1, canvas=(64, 64), content=(21, 19), tl=_TL, br=_BR),
    "reflect64_n8": dict(family="reflect", conv=S1, canvas=(64, 64), content=(21, 19), tl=_TL[:3], br=_BR[:3]),
    # 7 x 7 layers, four images: both corners and one extension each
    "reflect7_256": dict(family="reflect", conv=S1K7, canvas=(256, 256), content=(37, 41), tl=[(12, 30)], br=[(33, 15)]),
    "reflect7_128x160": dict(family="reflect", conv=S1K7, canvas=(128, 160), content=(37, 41), tl=[(12, 30)], br=[(33, 15)]),
    "zero_s2k7": dict(family="zero", conv=S2K7, canvas=(256, 256), content=(37, 41), offsets=[(0, 0), (218, 214), (30, 2), (2, 30)]),
    # the 4 x 4 kernels (PatchGAN discriminator, U-Net up-convs): zero padding only
    "zero_s2k4": dict(family="zero", conv=S2K4, canvas=(74, 91), content=(37, 35),
                      offsets=[(2 * y, 2 * x) for y, x in [(0, 0), (18, 27), (15, 1), (1, 15), (16, 17), (2, 16), (10, 9), (17, 22)]]),
    "zero_s1k4": dict(family="zero", conv=S1K4, canvas=(34, 38), content=(21, 19), offsets=[(0, 0), (13, 19), (11, 15), (12, 1), (1, 13), (5, 16), (8, 7), (3, 10)]),
    "zero_t4": dict(family="zero", conv=T4, canvas=(35, 37), content=(11, 13), offsets=[(0, 0), (24, 24), (15, 1), (1, 15), (16, 17), (5, 16), (20, 8), (8, 20)]),
    "roll64_n16": dict(family="roll", conv=S1, canvas=(64, 64), shifts=_ROLL),
    "roll64_n8": dict(family="roll", conv=S1, canvas=(64, 64), shifts=_ROLL[:8]),
}


def place(name, content, depth=None):
    """(batch, pairs) of PLACEMENTS[name] for a content [C][h][w] of the placement's size (the roll family: a whole image)"""
    pl = PLACEMENTS[name]
    want = pl["canvas"] if pl["family"] == "roll" else pl["content"]
    if tuple(content.shape[1:]) != tuple(want):
        raise ValueError("%s takes a content of %s" % (name, want))
    if pl["family"] == "zero":
        return zero_canvas(content, pl["canvas"], pl["offsets"], pl["conv"])
    if pl["family"] == "reflect":
        return reflect_border(content, pl["canvas"], pl["conv"].pad, pl["tl"], pl["br"])
    return roll_family(content, pl["shifts"], pl["conv"].pad if depth is None else depth)


# ---- what a list of pairs covers

def positions(pairs):
    """the patch-relative positions (y mod 16, x mod 16) of the compared outputs, on the side of the image that is not the reference"""
    return {((p.y + i) % PATCH, (p.x + j) % PATCH) for p in pairs for i in range(min(p.h, PATCH)) for j in range(min(p.w, PATCH))}


def edge_residues(pairs):
    """({top and bottom window edges mod 16}, {left and right ones}) over both sides of every pair; an edge is the first row (column) of a
    window and the first one behind it"""
    ys = {e % PATCH for p in pairs for e in (p.y, p.y + p.h, p.ry, p.ry + p.h)}
    xs = {e % PATCH for p in pairs for e in (p.x, p.x + p.w, p.rx, p.rx + p.w)}
    return ys, xs


def corners_used(pairs, out_hw):
    """a window starts at the output's (0, 0) and one ends at its (H, W)"""
    wins = [(p.y, p.x, p.h, p.w) for p in pairs] + [(p.ry, p.rx, p.h, p.w) for p in pairs]
    return any(y == 0 and x == 0 for y, x, h, w in wins) and any(y + h == out_hw[0] and x + w == out_hw[1] for y, x, h, w in wins)


def outputs_compared(pairs, channels):
    return channels * sum(p.h * p.w for p in pairs)


# ---- the comparison

class Report:
    """result of compare(): .ok, .compared (outputs), .positions (patch-relative positions covered), and per blamed image
    .images[k] = dict(count, rel, hist [16][16], chan [64])"""

    def __init__(self, compared, npos):
        self.compared, self.positions, self.images = compared, npos, {}

    @property
    def ok(self):
        return not self.images

    def _entry(self, k):
        return self.images.setdefault(k, dict(count=0, rel=0.0, hist=torch.zeros(PATCH, PATCH, dtype=torch.long), chan=torch.zeros(64, dtype=torch.long)))

    def blame(self, k, y, x, bad, d, ref):
        """bad [C][h][w] bool: the outputs of image k's window at (y, x) that are wrong"""
        if not bool(bad.any()):
            return
        e = self._entry(k)
        e["count"] += int(bad.sum())
        e["rel"] = max(e["rel"], float((d.abs() / ref.abs().clamp_min(1e-30))[bad].max()))
        c, h, w = bad.shape
        per_px = bad.sum(0)
        yy = ((torch.arange(h) + y) % PATCH)[:, None].expand(h, w)
        xx = ((torch.arange(w) + x) % PATCH)[None, :].expand(h, w)
        e["hist"].view(-1).index_add_(0, (yy * PATCH + xx).reshape(-1), per_px.reshape(-1))
        e["chan"].index_add_(0, torch.arange(c) % 64, bad.sum((1, 2)))

    def summary(self):
        if self.ok:
            return "%d outputs compared, %d of 256 patch-relative positions covered, all equal" % (self.compared, self.positions)
        lines = ["%d outputs compared, %d of 256 patch-relative positions covered; differing:" % (self.compared, self.positions)]
        for k in sorted(self.images):
            e = self.images[k]
            rows = [i for i in range(PATCH) if int(e["hist"][i].sum())]
            cols = [j for j in range(PATCH) if int(e["hist"][:, j].sum())]
            chans = [c for c in range(64) if int(e["chan"][c])]
            top = sorted(((int(e["hist"][i, j]), i, j) for i in rows for j in cols if int(e["hist"][i, j])), reverse=True)[:6]
            lines.append("  image %d: %d outputs, max |d| / |ref| %.3g; %d of 256 patch positions, patch rows %s, patch columns %s, %d of 64 channel residues%s; most at (y, x) %s"
                         % (k, e["count"], e["rel"], int((e["hist"] > 0).sum()), rows, cols, len(chans), "" if len(chans) > 8 else " %s" % chans,
                            ", ".join("(%d, %d): %d" % (i, j, n) for n, i, j in top)))
        return "\n".join(lines)


def compare(out, pairs):
    """out [N][C][H][W] (any device).  Values are compared (torch.equal / !=: -0 equals +0).  Pairs that share a reference window form a
    group; in a group of three or more windows the value most of them agree on decides which image is blamed for a difference (so a fault
    under the REFERENCE's patch position is not charged to every other image), in a group of two both are."""
    out = out.detach().cpu()
    rep = Report(outputs_compared(pairs, out.shape[1]), len(positions(pairs)))
    groups = collections.OrderedDict()
    for p in pairs:
        groups.setdefault((p.ref, p.ry, p.rx, p.h, p.w), []).append(p)
    for (ref, ry, rx, h, w), members in groups.items():
        rwin = out[ref, :, ry:ry + h, rx:rx + w]
        wins = [out[p.img, :, p.y:p.y + h, p.x:p.x + w] for p in members]
        if all(torch.equal(win, rwin) for win in wins):
            continue
        where = [(ref, ry, rx)] + [(p.img, p.y, p.x) for p in members]
        stack = torch.stack([rwin] + wins)
        if len(where) >= 3:
            good = torch.mode(stack, 0).values
            for (k, y, x), win in zip(where, stack):
                rep.blame(k, y, x, win != good, win - good, good)
        else:
            bad = stack[0] != stack[1]
            rep.blame(where[0][0], where[0][1], where[0][2], bad, stack[0] - stack[1], stack[1])
            rep.blame(where[1][0], where[1][1], where[1][2], bad, stack[1] - stack[0], stack[0])
    return rep
