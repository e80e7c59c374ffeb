"""gdt_map_loss (gandtr_amd/csrc/map_loss.hip) against numpy float64, at the smallest shapes at which it can go wrong: counts around one chunk of 8192
values, images below and above a chunk, both kinds, the constant target, the sigmoid flag, several pairs of different sizes in one call -- and its
properties, each bit for bit: two runs, a pair alone against the pair in a group, a 4-byte-aligned view against the 16-byte-aligned copy, the total
against its definition.

Tolerance: every term is >= 0 and evaluated in float64 like the reference's, so a different order of additions moves a mean by at most count * 2^-53
relative; the sigmoid's own rounding (exp, the sum, the quotient: values <= 1) adds 2^-52.  Measured on an MI355X: at most 2.5e-16 relative on every case (the bound allows 4e-15 .. 6e-12)."""
import numpy as np
import pytest
import torch

from gandtr_amd.components.optim.criterion import compound
from gandtr_amd.tools import synth

pytestmark = pytest.mark.gpu

CHUNK = 8192
EPS53 = 2.0 ** -53


def _maps(seed, n_images, per_image, scale=2.0):
    shape = (n_images, per_image)
    return synth._normal(seed, "ml.a", shape, scale), synth._normal(seed, "ml.b", shape, scale)


def _ref(a, b, kind, sigmoid):
    """(per-image means, pair mean) in numpy float64; b an array or a number"""
    x = a.numpy().astype(np.float64)
    y = b.numpy().astype(np.float64) if torch.is_tensor(b) else np.float64(b)
    if sigmoid:
        x = 1.0 / (1.0 + np.exp(-x))
        if torch.is_tensor(b):
            y = 1.0 / (1.0 + np.exp(-y))
    term = np.abs(x - y) if kind == "l1" else (x - y) ** 2
    return term.mean(axis=1), term.mean()


def _check(got, a, b, kind, sigmoid, k=0):
    per_image, mean = _ref(a, b, kind, sigmoid)
    extra = 2.0 ** -52 if sigmoid else 0.0
    per = a.shape[1]
    err_img = np.abs(got.per_image[k].cpu().numpy() - per_image)
    assert got.per_image[k].dtype == torch.float64 and (err_img <= per * EPS53 * per_image + extra).all(), (err_img / np.maximum(per_image, 1e-300)).max()
    err = abs(float(got.per_pair[k].cpu()) - mean)
    print("count %d x %d %s sigmoid %d: |d| / mean = %.2e (allowed %.2e)" % (a.shape[0], per, kind, sigmoid, err / max(mean, 1e-300), a.numel() * EPS53))
    assert err <= a.numel() * EPS53 * mean + extra


COUNTS = [(1, 1), (1, 3), (1, 5), (1, CHUNK - 1), (1, CHUNK), (1, CHUNK + 1), (1, 3 * CHUNK + 3), (2, 35), (7, 35), (2, CHUNK + 5), (7, CHUNK + 5)]


@pytest.mark.parametrize("n_images,per_image", COUNTS)
def test_both_kinds_against_numpy_float64(cuda_device, n_images, per_image):
    a, b = _maps(n_images * 100003 + per_image, n_images, per_image)
    ad, bd = a.to(cuda_device), b.to(cuda_device)
    for kind in ("l1", "mse"):
        got = compound.map_losses([compound.MapPair(ad, bd, kind, False, 1.0)])
        assert got.per_pair.is_cuda and got.per_pair.dtype == torch.float64 and got.total.dim() == 0
        _check(got, a, b, kind, False)
        assert float(got.total.cpu()) == float(got.per_pair[0].cpu())
        crit = compound.GAN_CRITERIA[kind]()
        single = crit(ad, bd)                                                         # the criterion's 0-dim fp32 view
        assert single.is_cuda and single.dtype == torch.float32 and single.dim() == 0
        assert abs(float(single.cpu()) - float(got.per_pair[0].cpu())) <= 2.0 ** -24 * float(got.per_pair[0].cpu())
        total = compound.GAN_CRITERIA[kind](reduction="sum")(ad, bd)
        assert abs(float(total.cpu()) - float(got.per_pair[0].cpu()) * a.numel()) <= 2.0 ** -23 * float(total.cpu())


@pytest.mark.parametrize("n_images,per_image", [(1, 5), (7, 35), (1, CHUNK + 1), (2, CHUNK + 5)])
def test_constant_target_and_sigmoid_flag(cuda_device, n_images, per_image):
    a, b = _maps(n_images * 7919 + per_image, n_images, per_image, scale=12.0)
    a, b = a.clamp(-30.0, 30.0), b.clamp(-30.0, 30.0)
    a[0, 0], b[0, 0] = 30.0, -30.0                                                    # the ends of the range are in every case
    ad, bd = a.to(cuda_device), b.to(cuda_device)
    got = compound.map_losses([compound.MapPair(ad, 1.0, "mse", False, 1.0), compound.MapPair(ad, 0.0, "l1", False, 1.0),
                               compound.MapPair(ad, bd, "l1", True, 1.0), compound.MapPair(ad, bd, "mse", True, 1.0),
                               compound.MapPair(ad, 0.25, "l1", True, 1.0)])
    _check(got, a, 1.0, "mse", False, 0)
    _check(got, a, 0.0, "l1", False, 1)
    _check(got, a, b, "l1", True, 2)
    _check(got, a, b, "mse", True, 3)
    _check(got, a, 0.25, "l1", True, 4)                                               # the sigmoid never touches the constant


def _five(dev):
    shapes = ((3, 35), (1, CHUNK + 1), (2, 2 * CHUNK + 7), (7, 5), (1, 1))
    kinds = ("l1", "mse", "l1", "mse", "l1")
    sig = (False, False, True, False, True)
    weights = (1.0, 10.0, 5.0, 0.5, 0.1)
    host = [_maps(900 + i, *s) for i, s in enumerate(shapes)]
    pairs = [compound.MapPair(a.to(dev), b.to(dev), k, s, w) for (a, b), k, s, w in zip(host, kinds, sig, weights)]
    return host, pairs


def test_five_pairs_of_different_sizes_in_one_call(cuda_device):
    host, pairs = _five(cuda_device)
    got = compound.map_losses(pairs)
    assert got.per_pair.shape == (5,) and [t.numel() for t in got.per_image] == [3, 1, 2, 7, 1]
    for k, ((a, b), p) in enumerate(zip(host, pairs)):
        _check(got, a, b, p.kind, p.sigmoid, k)
    again = compound.map_losses(pairs)                                                # two runs of one call
    assert torch.equal(got.per_pair, again.per_pair) and torch.equal(got.total, again.total)
    assert all(torch.equal(x, y) for x, y in zip(got.per_image, again.per_image))
    for k, p in enumerate(pairs):                                                     # a pair alone against the pair in the group
        alone = compound.map_losses([p])
        assert torch.equal(alone.per_pair[0], got.per_pair[k]) and torch.equal(alone.per_image[0], got.per_image[k])
    reordered = compound.map_losses(pairs[::-1])
    assert torch.equal(reordered.per_pair.flip(0), got.per_pair)
    total = 0.0                                                                       # the total against its definition, in float64, in index order
    for p, v in zip(pairs, got.per_pair.cpu().tolist()):
        total += p.weight * v
    assert float(got.total.cpu()) == total


@pytest.mark.parametrize("n_images,per_image", [(1, 3), (2, 35), (1, CHUNK), (3, CHUNK + 5), (1, 3 * CHUNK + 3)])
def test_a_shifted_view_gives_the_bits_of_the_aligned_copy(cuda_device, n_images, per_image):
    a, b = _maps(n_images * 31 + per_image, n_images, per_image)
    count = a.numel()
    ad, bd = a.to(cuda_device), b.to(cuda_device)
    assert ad.data_ptr() % 16 == 0 and bd.data_ptr() % 16 == 0
    shifted = []
    for t, shift in ((ad, 1), (bd, 3)):
        buf = torch.empty(count + 4, dtype=torch.float32, device=cuda_device)
        view = buf[shift:shift + count].view(n_images, per_image)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 * shift and view.is_contiguous()
        shifted.append(view)
    for kind, sig in (("l1", False), ("mse", False), ("l1", True)):
        base = compound.map_losses([compound.MapPair(ad, bd, kind, sig, 1.0)])
        for x, y in ((shifted[0], bd), (ad, shifted[1]), (shifted[0], shifted[1])):
            moved = compound.map_losses([compound.MapPair(x, y, kind, sig, 1.0)])
            assert torch.equal(moved.per_pair, base.per_pair) and torch.equal(moved.per_image[0], base.per_image[0])


def test_refusals_on_the_device(cuda_device):
    a = torch.zeros((2, 8), device=cuda_device)
    with pytest.raises(ValueError):
        compound.map_losses([compound.MapPair(a, a[:, :4], "l1", False, 1.0)])
    with pytest.raises(ValueError):
        compound.map_losses([compound.MapPair(a, a, "l1", False, 1.0)] * 17)
    with pytest.raises(ValueError):
        compound.map_losses([compound.MapPair(a, a.cpu(), "l1", False, 1.0)])
    with pytest.raises(NotImplementedError):
        compound.map_losses([compound.MapPair(a, a, "bce", False, 1.0)])
    assert float(compound.L1Loss()(a, a).cpu()) == 0.0
    assert compound.L1Loss(reduction="none")(a, a + 1).shape == a.shape              # "none": plain torch ops
