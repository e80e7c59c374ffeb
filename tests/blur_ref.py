"""Shared by the tests of the anti-aliased sampling (gdt_net_blur_resample, csrc/blur_resample.hip): float64 evaluations of the two ops from their definitions, with
and without the producer's InstanceNorm (+ ReLU) applied first, fp32 emulations of a correct kernel and of wrong ones, the cases, and the reader of the
gen_tiny_aa_* fixtures (no test in here).

Downsample: reflection pad by 1 (without the edge pixel), then per axis the taps (1, 2, 1) / 4 at stride 2 -- out[o] = (x[r(2 o - 1)] + 2 x[2 o] + x[r(2 o + 1)]) / 4,
ceil(n / 2) outputs, n >= 2.  Upsample: per axis out[2 i] = 0.25 x[max(i - 1, 0)] + 0.75 x[i], out[2 i + 1] = 0.75 x[i] + 0.25 x[min(i + 1, n - 1)].  Both are
separable and linear with non-negative weights that sum to one, so the same routine gives the value, the weighted sum of magnitudes and a carried error.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

import conv_bound as cb

EPS_NORM = float(np.float32(1e-5))
NORMS = (None, "plain", "relu")             # the op alone; InstanceNorm in front of it; InstanceNorm + ReLU


# ---- index tables: per axis, output o = sum_k weight[k] * x[index[k][o]] ----------------------------------------------------------------------------------------------
def reflect(i, n):
    """index of a reflection padding without the edge pixel, any distance (period 2 (n - 1))"""
    p = 2 * (n - 1)
    j = np.mod(i, p)
    return np.where(j >= n, p - j, j)


def down_axis(n, pad="reflect", parity=0):
    """(indices [3][ceil(n / 2)], weights [3]); ``pad``: "reflect" (the layer), "replicate" or "zero" (index -1: a zero tap); ``parity`` 1: the window one pixel late"""
    o = np.arange((n + 1) // 2)
    raw = np.stack([2 * o - 1 + parity, 2 * o + parity, 2 * o + 1 + parity])
    if pad == "reflect":
        idx = reflect(raw, n)
    elif pad == "replicate":
        idx = np.clip(raw, 0, n - 1)
    else:
        idx = np.where((raw < 0) | (raw >= n), -1, raw)
    return idx, (0.25, 0.5, 0.25)


def up_axis(n, pad="replicate", swap=False):
    """(indices [2][2 n], weights [2]): tap 0 = the pixel itself (0.75), tap 1 = its neighbour on the output's side (0.25); ``swap``: the two weights exchanged"""
    o = np.arange(2 * n)
    i = o // 2
    nb = np.where(o % 2 == 0, i - 1, i + 1)
    if pad == "replicate":
        nb = np.clip(nb, 0, n - 1)
    elif pad == "reflect":
        nb = reflect(nb, n) if n > 1 else np.zeros_like(nb)
    else:
        nb = np.where((nb < 0) | (nb >= n), -1, nb)
    return np.stack([i, nb]), ((0.25, 0.75) if swap else (0.75, 0.25))


def _gather(v, idx, dim):
    """v indexed along ``dim`` by ``idx`` (-1: zero)"""
    t = v.index_select(dim, torch.from_numpy(np.maximum(idx, 0)))
    if (idx < 0).any():
        shape = [1] * v.dim()
        shape[dim] = -1
        t = t * torch.from_numpy((idx >= 0).astype(np.float64)).to(v.dtype).reshape(shape)
    return t


def apply_axes(v, ay, ax):
    """sum_kl wy[k] wx[l] v[iy[k], ix[l]] in v's dtype (float64 for the references)"""
    (iy, wy), (ix, wx) = ay, ax
    rows = sum(w * _gather(v, iy[k], 2) for k, w in enumerate(wy))
    return sum(w * _gather(rows, ix[k], 3) for k, w in enumerate(wx))


def axes(shape, up, **kw):
    h, w = shape[2:]
    return (up_axis(h, **kw), up_axis(w, **kw)) if up else (down_axis(h, **kw), down_axis(w, **kw))


def normalise(x, relu, eps=EPS_NORM):
    """float64 InstanceNorm2d(affine=False) (+ ReLU) of x"""
    x = x.double()
    z = (x - x.mean(dim=(2, 3), keepdim=True)) / torch.sqrt(x.var(dim=(2, 3), unbiased=False, keepdim=True) + eps)
    return F.relu(z) if relu else z


def blur(x, up, norm=None):
    """float64 value of the op on the tensor ``x`` it consumed; ``norm`` "plain" / "relu": of InstanceNorm (+ ReLU) of x, which the folded form never stores"""
    v = x.double() if norm is None else normalise(x, norm == "relu")
    return apply_axes(v, *axes(x.shape, up))


# ---- fp32 emulations ----------------------------------------------------------------------------------------------------------------------------------------------------
FAULTS_DOWN = ("zero_pad", "replicate", "parity")
FAULTS_UP = ("zero_pad", "reflect", "phase_swap")
FAULTS_NORM = ("relu_after", "neighbour_stats")        # relu_after: the ReLU form only


def emulate(x, up, norm=None, out_f32=False, fault=None):
    """the kernel in fp32 on the CPU, in its own order: the horizontal pass per row, then the vertical one; down (a + 2 b) + c twice and one exact scaling, up
    0.75 a + 0.25 b per axis rounded once (the kernel's fma); a folded norm as (x - mean') * rstd' with the statistics conv_bound.emulate_stats takes from x.
    ``fault``: a wrong kernel -- zero padding; replicate for reflect (down); reflect for replicate (up); the 0.25 / 0.75 phases exchanged (up); the window one pixel
    late (down); the ReLU behind the blur instead of in front of it; the statistics of the neighbouring image (of the neighbouring channel when there is one image)"""
    v = x.float()
    n, c, h, w = v.shape
    if norm is not None:
        mean, rstd = cb.emulate_stats(v, rows=min(h * w, 1024))
        if fault == "neighbour_stats":
            shift = (1, 0) if n > 1 else (0, 1)
            mean, rstd = mean.roll(shift, (0, 1)), rstd.roll(shift, (0, 1))
        v = (v - mean.float()[:, :, None, None]) * rstd.float()[:, :, None, None]
        if norm == "relu" and fault != "relu_after":
            v = F.relu(v)
    kw = {}
    if fault == "zero_pad":
        kw["pad"] = "zero"
    elif fault in ("replicate", "reflect"):
        kw["pad"] = fault
    elif fault == "parity":
        kw["parity"] = 1
    elif fault == "phase_swap":
        kw["swap"] = True
    (iy, wy), (ix, wx) = axes(v.shape, up, **kw)
    if up:
        lerp = lambda a, b, wa, wb: (wa * a.double() + wb * b.double()).float()
        rows = lerp(_gather(v, ix[0], 3), _gather(v, ix[1], 3), wx[0], wx[1])
        o = lerp(_gather(rows, iy[0], 2), _gather(rows, iy[1], 2), wy[0], wy[1])
    else:
        rows = (_gather(v, ix[0], 3) + 2.0 * _gather(v, ix[1], 3)) + _gather(v, ix[2], 3)
        o = ((_gather(rows, iy[0], 2) + 2.0 * _gather(rows, iy[1], 2)) + _gather(rows, iy[2], 2)) * 0.0625
    if norm == "relu" and fault == "relu_after":
        o = F.relu(o)
    return o if out_f32 else cb.f16(o)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------------------------------------
# (N, C, H, W) of the tensor the op reads: the smallest at which each thing can go wrong
SHAPES = [(2, 8, 2, 2),         # both reflections land on the same pixel; one channel vector
          (2, 8, 2, 3),
          (1, 16, 5, 7),        # odd sizes: the last window hangs into the pad
          (2, 64, 16, 16),      # 256 pixels: the producing conv delivers the statistics from its epilogue
          (1, 256, 9, 4),       # many vectors per pixel
          (2, 32, 37, 53)]      # more than one workgroup, more than one row chunk, ragged
SHAPES_UP_ONLY = [(1, 8, 1, 4), (2, 8, 3, 1)]
BIAS_STD = 1.0                  # of the producing 1 x 1 conv's bias: channel means up to about 2 standard deviations


def cases():
    return [(s, False) for s in SHAPES] + [(s, True) for s in SHAPES + SHAPES_UP_ONLY]


def case_id(case):
    shape, up = case
    return ("up-" if up else "down-") + "x".join(str(e) for e in shape)


def producer_weights(c):
    from gandtr_amd.tools import synth
    return synth._normal(21, "w", (c, 3, 1, 1), 0.7), synth._normal(21, "b", (c,), BIAS_STD)


def producer_input(shape):
    from gandtr_amd.tools import synth
    return synth.synth_input(21, (shape[0], 3, shape[2], shape[3]))


def fused_statistics(shape):
    """whether the producing conv hands the norm its statistics from its epilogue (conv_fuses_stats, net_plan.hip): output pixels a multiple of 128"""
    return (shape[2] * shape[3]) % 128 == 0


# ---- the gen_tiny_aa_* fixtures (tests/golden/make_antialias_golden.py) -------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_taps(name, prefix=""):
    """(layers, {tap index: float32 tensor of the first ``images`` images of the batch}) of a fixture file: the taps stored under their own index or under the index of
    an identical tensor (the in-place ReLUs); the two reflection-padded tensors and the taps a file leaves out are absent"""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    layers = int(g[prefix + "layers"])
    same_as = g[prefix + "same_as"]
    return layers, {i: torch.from_numpy(g["%stap%d" % (prefix, same_as[i])]) for i in range(layers) if same_as[i] >= 0}
