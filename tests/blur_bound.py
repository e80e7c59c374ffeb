"""Per-element bounds for the anti-aliased sampling ops (csrc/blur_resample.hip) against the float64 evaluations of blur_ref.py, derived from the arithmetic in the
manner of aux_bound.py (no test in here).  u = 2^-24, g_k = k u / (1 - k u).

* The weights are exact.  Down: (1, 2, 1) x (1, 2, 1) / 16 are powers of two, so all nine products are exact and only the eight additions round, in whatever order
  (separable or not): |d| <= g_8 sum_k w_k |t_k|.  Up: 9/16, 3/16, 3/16, 1/16 as products of 0.75 and 0.25; a term passes at most two roundings as a product (one
  per axis, none where the kernel fuses) and the four terms meet in three additions: |d| <= g_5 sum_k w_k |t_k| covers every order and every contraction.
* Folded form: a tap is t = (x - mean') * rstd' (+ ReLU, 1-Lipschitz) instead of the float64 z: |t - z| <= dz = |z| e_r + e_m (1 + e_r) + 2 u (|x| + |mean|) rstd
  (conv_bound.norm_value), with (e_r, e_m) from statistics_errors() below.  The op is a convex combination, so it carries blur(dz), and the magnitudes in the
  arithmetic term grow by it.
* Store: the fp32 tensors of f16x3 / f16c hold the fp32 result as it is (its last rounding is one of the g_k); fp16: 2^-11 (|ref| + e) + 2^-25.

statistics_errors(): aux_bound.stat_errors bounds the statistics the device takes from the STORED tensor.  Where the producing conv delivers them from its epilogue
(output pixels a multiple of 128) they are sums over 128-pixel tiles of the conv's fp32 results y BEFORE the store, and the stored fp16 tensor x the reference sees
is fl16(y): |y - x| <= rho |x| + 2^-25 with rho = 2^-11 / (1 - 2^-11) (rho = 0 for fp32 tensors).  With A1 = mean |x|, A2 = mean x^2, g = g_(k+1) of the chunk:
    mean:      |m' - m| <= g (1 + rho) A1 + rho A1 + 2^-25 + u |m|
    variance:  |var' - var| <= (g (1 + rho)^2 + 2 rho + rho^2) A2 + 2 |m| dm + dm^2  (+ the subnormal term, < 1e-7 of it)
    rstd:      as in aux_bound.stat_errors.
rho A1 / std is ~1e-3 for channel means of 2 standard deviations: this worst case (every rounding in the same direction) is far above what 256 roundings do
(measured figures: test_hip_blur_resample.py), and it only matters where the result is near zero; elsewhere the fp16 store's own 2^-11 dominates.
"""
import torch

import aux_bound as ab
import blur_ref as br
import conv_bound as cb
from aux_bound import Ref, assert_within, gamma, ratio    # noqa: F401  (re-exported for the tests)
from conv_bound import SUB16, U16, U32

RHO16 = U16 / (1 - U16)


def statistics_errors(x, fused=False, out_f32=True, eps=br.EPS_NORM):
    """(e_r, e_m) per (n, c) [N, C, 1, 1]: relative error of rstd, error of the mean in standard deviations.  ``fused`` with fp16 tensors: the statistics are those of
    the conv's results before their store (see the module docstring); else aux_bound.stat_errors (the chunk is then the 128-pixel tile or the 1024-pixel chunk of the
    separate pass: the longer one bounds both)"""
    if not fused or out_f32:
        return ab.stat_errors(x, eps)
    x = x.double()
    g, rho = gamma(ab.chunk_len(x.shape[2] * x.shape[3]) + 1), RHO16
    m = x.mean(dim=(2, 3), keepdim=True)
    var = x.var(dim=(2, 3), unbiased=False, keepdim=True)
    a1, a2 = x.abs().mean(dim=(2, 3), keepdim=True), (x * x).mean(dim=(2, 3), keepdim=True)
    dm = g * (1 + rho) * a1 + rho * a1 + SUB16 + U32 * m.abs()
    dvar = (g * (1 + rho) ** 2 + 2 * rho + rho ** 2) * a2 * (1 + 1e-7) + 2 * m.abs() * dm + dm ** 2
    t = dvar / (var + eps)
    assert float(t.max()) < 0.5, float(t.max())
    return 1.0 / torch.sqrt(1 - t) - 1 + U32, dm / torch.sqrt(var + eps)


def blur(x, up, norm=None, out_f32=False, fused=False):
    """Ref(float64 value, bound) of the op on the tapped tensor ``x``; ``norm`` None / "plain" / "relu": the producer's InstanceNorm (+ ReLU) folded in, evaluated
    from the RAW tensor; ``fused``: blur_ref.fused_statistics of the shape"""
    ay, ax = br.axes(x.shape, up)
    k = 5 if up else 8
    if norm is None:
        a, dz = x.double(), None
    else:
        e_r, e_m = statistics_errors(x, fused, out_f32)
        a, dz = cb.norm_value(x, relu=norm == "relu", err_r=e_r, err_m=e_m)
    ref, mag = br.apply_axes(a, ay, ax), br.apply_axes(a.abs(), ay, ax)
    carried = br.apply_axes(dz, ay, ax) if dz is not None else torch.zeros_like(ref)
    e = carried + gamma(k) * (mag + carried)
    return Ref(ref, e if out_f32 else e + U16 * (ref.abs() + e) + SUB16)


def resize_x2(x, out_f32=False):
    """Ref of gdt_k_resize (bilinear) at exactly twice the size: the same function; its coordinates are exact rationals there (lambda = 0.25 / 0.75), so of
    aux_bound.bilinear's terms only the weights' and the arithmetic's remain: (2 + 2 + 8) u max |tap| <= 12 u max over the 3 x 3 neighbourhood's taps -- here the
    weighted sum is bounded by the largest tap, taken as the up op's own taps"""
    ay, ax = br.axes(x.shape, True)
    v = x.double()
    ref = br.apply_axes(v, ay, ax)
    taps = torch.stack([br._gather(br._gather(v.abs(), ay[0][k], 2), ax[0][l], 3) for k in range(2) for l in range(2)]).max(0).values
    e = 12 * U32 * taps
    return Ref(ref, e if out_f32 else e + U16 * (ref.abs() + e) + SUB16)
