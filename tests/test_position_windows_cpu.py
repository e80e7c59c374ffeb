"""tests/position_windows.py on the CPU: the window arithmetic with exactly summable data (integers in float64: F.conv2d and
F.conv_transpose2d give the same number in any summation order), the coverage conditions on every placement the device tests run, and
an injected position-dependent fault that the report must locate."""
import pytest
import torch
import torch.nn.functional as F

import position_windows as PW
from position_windows import PLACEMENTS, S1


def _ints(seed, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).double()


def _conv(x, wt, conv, reflect=False):
    if conv.transposed:
        return F.conv_transpose2d(x, wt, stride=conv.stride, padding=conv.pad, output_padding=conv.opad)
    if reflect:
        return F.conv2d(F.pad(x, (conv.pad,) * 4, mode="reflect"), wt, stride=conv.stride)
    return F.conv2d(x, wt, stride=conv.stride, padding=conv.pad)


def _weights(seed, conv, cin, cout, lo=-3, hi=3):
    return _ints(seed, (cin, cout, conv.k, conv.k) if conv.transposed else (cout, cin, conv.k, conv.k), lo, hi)


def _content(name, seed=1, c=4, lo=-4, hi=4):
    pl = PLACEMENTS[name]
    return _ints(seed, (c,) + tuple(pl["canvas"] if pl["family"] == "roll" else pl["content"]), lo, hi)


ZERO = [n for n, pl in PLACEMENTS.items() if pl["family"] == "zero" and not pl.get("inner")]     # (inner: a reflect layer, see its own test below)
REFLECT = [n for n, pl in PLACEMENTS.items() if pl["family"] == "reflect"]
ROLL = [n for n, pl in PLACEMENTS.items() if pl["family"] == "roll"]


@pytest.mark.parametrize("name", list(PLACEMENTS))
def test_every_pair_of_windows_is_equal_on_exactly_summable_data(name):
    pl = PLACEMENTS[name]
    conv = pl["conv"]
    batch, pairs = PW.place(name, _content(name))
    reflect = pl["family"] != "zero" or pl.get("inner", False)
    out = _conv(batch, _weights(2, conv, 4, 6), conv, reflect)
    assert out.shape[2:] == (PW.out_size(conv, pl["canvas"][0]), PW.out_size(conv, pl["canvas"][1]))
    rep = PW.compare(out, pairs)
    assert rep.ok, rep.summary()
    assert rep.compared == 6 * sum(p.h * p.w for p in pairs) > 0
    assert len(pairs) >= len(batch) - 1 and {p.img for p in pairs} == set(range(1, len(batch)))       # every image but image 0 is compared


@pytest.mark.parametrize("name", ZERO)
def test_zero_canvas_windows_leave_out_only_what_they_must(name):
    """positive data: an output is non-zero exactly where it reads a content pixel.  Every output of the window does; outside the touched
    range (window + margin) nothing does; and the margin -- outputs beside the content that still read it -- is left out because the image
    in the canvas corner has no such outputs: they lie off the canvas"""
    pl = PLACEMENTS[name]
    conv = pl["conv"]
    content = _content(name, lo=1, hi=4)
    batch, pairs = PW.place(name, content)
    out = _conv(batch, _weights(2, conv, 4, 6, 1, 3), conv)
    h, w = pl["content"]
    oh, ow = out.shape[2:]
    margins = set()
    for k, (dy, dx) in enumerate(pl["offsets"]):
        (y, wh), (x, ww) = PW.window(conv, dy, h), PW.window(conv, dx, w)
        (ty, th), (tx, tw) = PW.touched(conv, dy, h), PW.touched(conv, dx, w)
        assert ty <= y and ty + th >= y + wh and tx <= x and tx + tw >= x + ww
        margins.add((y - ty, ty + th - y - wh, x - tx, tx + tw - x - ww))
        assert bool((out[k, :, y:y + wh, x:x + ww] != 0).all())
        mask = torch.zeros(oh, ow, dtype=torch.bool)
        mask[max(ty, 0):max(ty + th, 0), max(tx, 0):max(tx + tw, 0)] = True
        assert bool((out[k][:, ~mask] == 0).all()) and bool((out[k][:, mask] != 0).all())
    assert len(margins) == 1                                      # the same margin at every offset: it depends on the conv alone
    top, bottom, left, right = margins.pop()
    (y0, _), (x0, _) = PW.window(conv, pl["offsets"][0][0], h), PW.window(conv, pl["offsets"][0][1], w)
    assert (top == 0 or y0 - top < 0) and (left == 0 or x0 - left < 0)             # image 0 (top-left corner): no outputs above / left of its window
    ends = [(PW.window(conv, dy, h), PW.window(conv, dx, w)) for dy, dx in pl["offsets"]]
    assert any((bottom == 0 or y + wh + bottom > oh) and (right == 0 or x + ww + right > ow) for (y, wh), (x, ww) in ends)


def test_inner_placement_keeps_clear_of_the_reflected_border():
    """zero canvas under a REFLECT layer: equal windows need the content one pixel off the canvas border (checked above with the reflect
    conv); at the border itself the layer mirrors the content into its own neighbourhood and the window differs"""
    pl = PLACEMENTS["zero64_inner"]
    assert all(1 <= dy <= 64 - 21 - 1 and 1 <= dx <= 64 - 19 - 1 for dy, dx in pl["offsets"])
    assert pl["offsets"][0] == (1, 1) and pl["offsets"][1] == (64 - 21 - 1, 64 - 19 - 1)
    batch, pairs = PW.zero_canvas(_content("zero64_inner", lo=1, hi=4), (64, 64), [(0, 0), (20, 20)], S1)
    assert not PW.compare(_conv(batch, _weights(2, S1, 4, 6, 1, 3), S1, reflect=True), pairs).ok


@pytest.mark.parametrize("name", REFLECT)
def test_reflect_pairing_covers_the_border_outputs_and_needs_the_extension(name):
    pl = PLACEMENTS[name]
    conv, (h, w), (hh, ww) = pl["conv"], pl["content"], pl["canvas"]
    content = _content(name, lo=1, hi=4)
    batch, pairs = PW.place(name, content)
    assert len(batch) == 2 + len(pl["tl"]) + len(pl["br"])
    # the corner windows are the whole content, border rows and columns included
    assert all((p.ry, p.rx, p.h, p.w) == (0, 0, h, w) for p in pairs if p.ref == 0 and p.img > 1)
    assert all((p.ry, p.rx, p.h, p.w) == (hh - h, ww - w, h, w) for p in pairs if p.ref == 1)
    assert sum(p.ref == 0 and p.img > 1 for p in pairs) == len(pl["tl"]) and sum(p.ref == 1 for p in pairs) == len(pl["br"])
    # without the host-side extension (plain content in the interior) the border outputs differ, and only those
    plain = batch.clone()
    k = 2
    for oy, ox in pl["tl"]:
        plain[k] = 0
        plain[k, :, oy + conv.pad:oy + conv.pad + h, ox + conv.pad:ox + conv.pad + w] = content
        k += 1
    rep = PW.compare(_conv(plain, _weights(2, conv, 4, 6, 1, 3), conv, reflect=True), pairs)
    assert not rep.ok and set(rep.images) <= set(range(2 + len(pl["tl"]))) and rep.images


@pytest.mark.parametrize("name", ROLL)
def test_roll_windows_leave_out_the_border_ring_and_the_seam(name):
    pl = PLACEMENTS[name]
    hh, ww = pl["canvas"]
    image = _content(name)
    batch, pairs = PW.place(name, image)
    for p in pairs:
        dy, dx = pl["shifts"][p.img]
        assert (p.y - p.ry) % hh == dy % hh and (p.x - p.rx) % ww == dx % ww
        assert 1 <= p.y and p.y + p.h <= hh - 1 and 1 <= p.ry and p.ry + p.h <= hh - 1
        assert 1 <= p.x and p.x + p.w <= ww - 1 and 1 <= p.rx and p.rx + p.w <= ww - 1
    for k in range(1, len(batch)):                   # what is left out: the ring, and the rows / columns whose neighbourhood crosses the seam
        dy, dx = pl["shifts"][k]
        rows = sum(p.h for p in pairs if p.img == k and p.x == min(q.x for q in pairs if q.img == k))
        cols = sum(p.w for p in pairs if p.img == k and p.y == min(q.y for q in pairs if q.img == k))
        assert rows == hh - len({0, hh - 1, (dy - 1) % hh, dy % hh}) and cols == ww - len({0, ww - 1, (dx - 1) % ww, dx % ww})
    # a pointwise tensor (depth 0): everything is compared
    _, flat = PW.place(name, image, depth=0)
    assert PW.outputs_compared(flat, 1) == (len(batch) - 1) * hh * ww
    assert PW.compare(batch * 3.0, flat).ok
    # with the ring or seam included the reflect conv differs there
    wide = [PW.Pair(p.img, p.y - 1, p.x, p.ref, p.ry - 1, p.rx, p.h + 2, p.w) for p in pairs]
    assert not PW.compare(_conv(batch, _weights(2, S1, 4, 6, 1, 3), S1, reflect=True), wide).ok


@pytest.mark.parametrize("name", list(PLACEMENTS))
def test_placements_meet_the_coverage_conditions(name):
    """per placement: all 256 patch-relative positions compared; a window edge on a multiple of 16, one a pixel before, one a pixel after
    (the transposed form's output windows start and end on even pixels: there the edges of the CONTENT, in the input's patch grid, meet the
    condition, and the output windows have edges on a multiple of 16, two before and two after); both canvas corners used"""
    pl = PLACEMENTS[name]
    conv = pl["conv"]
    batch, pairs = PW.place(name, _content(name))
    assert len(PW.positions(pairs)) == 256
    ys, xs = PW.edge_residues(pairs)
    if conv.transposed:
        assert {0, 2, 14} <= ys and {0, 2, 14} <= xs
        h, w = pl["content"]
        ys, xs = {e % 16 for dy, dx in pl["offsets"] for e in (dy, dy + h)}, {e % 16 for dy, dx in pl["offsets"] for e in (dx, dx + w)}
    assert {0, 1, 15} <= ys and {0, 1, 15} <= xs, (sorted(ys), sorted(xs))
    out_hw = (PW.out_size(conv, pl["canvas"][0]), PW.out_size(conv, pl["canvas"][1]))
    if pl["family"] == "roll":
        assert all(len({pl["shifts"][k][a] % 16 for k in range(len(batch))}) >= 7 for a in (0, 1))      # whole images: no corners; the shifts spread over the patch
    elif pl.get("inner"):
        assert not PW.corners_used(pairs, out_hw)              # (the reflect layer forbids them: test_inner_placement_keeps_clear_of_the_reflected_border)
    else:
        assert PW.corners_used(pairs, out_hw)
    assert len({tuple(pl[key][k]) for key in ("offsets", "shifts", "tl", "br") if key in pl for k in range(len(pl[key]))}) \
        == sum(len(pl[key]) for key in ("offsets", "shifts", "tl", "br") if key in pl)                     # every image its own place


def test_ragged_windows_reach_into_the_partial_patches():
    pl = PLACEMENTS["zero_ragged"]
    _, pairs = PW.place("zero_ragged", _content("zero_ragged"))
    wins = [(p.y, p.x, p.h, p.w) for p in pairs] + [(pairs[0].ry, pairs[0].rx, pairs[0].h, pairs[0].w)]
    assert pl["canvas"] == (76, 92)
    assert sum(y + h > 64 for y, x, h, w in wins) >= 3 and sum(x + w > 80 for y, x, h, w in wins) >= 3
    assert any(y + h > 64 and x + w > 80 for y, x, h, w in wins) and any(y < 64 < y + h for y, x, h, w in wins) and any(x < 80 < x + w for y, x, h, w in wins)


def _ring_faulty_conv(x, wt):
    """a patch kernel that stages the ring of every 16 x 16 patch wrongly: the inputs at patch rows / columns 0 and 15 come out changed by
    an amount that depends on where they are"""
    n, c, hh, ww = x.shape
    yy, xx = torch.arange(hh)[:, None] % 16, torch.arange(ww)[None, :] % 16
    ring = ((yy == 0) | (yy == 15) | (xx == 0) | (xx == 15)).double()
    where = (torch.arange(hh)[:, None] * 131 + torch.arange(ww)[None, :] * 17 + 1).double()
    return F.conv2d(x + ring * where * (x != 0), wt, padding=1)


def test_an_injected_fault_at_the_patch_ring_is_located():
    content = _content("zero64_n8", lo=1, hi=4)
    batch, pairs = PW.place("zero64_n8", content)
    wt = _weights(2, S1, 4, 6, 1, 3)
    assert PW.compare(F.conv2d(batch, wt, padding=1), pairs).ok
    rep = PW.compare(_ring_faulty_conv(batch, wt), pairs)
    assert not rep.ok and rep.compared == 6 * 7 * 21 * 19 and rep.positions == 256
    near = torch.zeros(16, 16, dtype=torch.bool)                  # outputs that read a ring pixel: patch rows / columns 0, 1, 14, 15
    near[[0, 1, 14, 15], :] = True
    near[:, [0, 1, 14, 15]] = True
    assert 0 in rep.images and len(rep.images) == 8              # the reference image is blamed for its own positions, not everybody else for them
    for k, e in rep.images.items():
        assert e["count"] == int(e["hist"].sum()) == int(e["chan"].sum()) > 0 and e["rel"] > 0
        assert int(e["hist"][~near].sum()) == 0, (k, e["hist"])  # nothing is charged to the patch interior
        assert int(e["hist"][near].sum()) > 0
    total = sum(e["hist"] for e in rep.images.values())
    assert bool((total[near] > 0).all())                          # and the whole neighbourhood of the ring shows
    text = rep.summary()
    assert all("image %d:" % k in text for k in range(8)) and "patch rows [" in text and "patch columns [" in text and "channel residues" in text
    # a fault in ONE output channel shows in the channel histogram
    out = F.conv2d(batch, wt, padding=1)
    out[3, 5, 20, 20] += 1.0
    rep = PW.compare(out, pairs)
    assert list(rep.images) == [3] and rep.images[3]["count"] == 1 and int(rep.images[3]["chan"][5]) == 1 and int(rep.images[3]["hist"][4, 4]) == 1
    # -0 and +0 are the same value
    z = torch.zeros(2, 1, 4, 4)
    z[1] = -0.0
    assert PW.compare(z, [PW.Pair(1, 0, 0, 0, 0, 0, 4, 4)]).ok
