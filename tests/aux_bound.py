"""Shared by test_aux_bound_cpu.py and test_hip_aux_ops.py: float64 references of the graph's non-conv ops (csrc/aux_kernels.hip) with a derived bound per output
element, and fp32 emulations of a correct kernel and of wrong ones (no test in here).

Every reference is evaluated on the tensor the op consumed (the tapped fp16 or fp32 tensor), so the producer's error is not in it.  Every bound is built from
u = 2^-24 (fp32 unit round-off: every fp32 operation returns its exact result times (1 + d), |d| <= u), g_k = k u / (1 - k u) (k roundings on one path, any
order), the fp16 store of conv_bound.py (2^-11 of the stored value, or half the subnormal spacing 2^-25) and the ulp figures of the math library the suite already
uses (tanhf 2 ulp, powf 16 ulp of 2^-23).  Each function's docstring derives its own terms.
"""
import collections
import math

import numpy as np
import torch
import torch.nn.functional as F

import conv_bound as cb
from conv_bound import SUB16, U16, U32

POWF_ULPS = 16.0                       # HIP math library: powf within 16 ulp (tests/test_hip_diffusion.py)
EPS_NORM = float(np.float32(1e-5))     # the fp32 constants the kernels receive, as the float64 numbers they are
EPS_POOL = float(np.float32(1e-6))

Ref = collections.namedtuple("Ref", "ref bound")


def gamma(k):
    return k * U32 / (1 - k * U32)


def ratio(got, r):
    """max |d| / bound (0 where d = 0; inf where the result is not finite)"""
    got = got.double()
    if tuple(got.shape) != tuple(r.ref.shape) or not bool(torch.isfinite(got).all()):
        return float("inf")
    d = (got - r.ref).abs()
    q = torch.where(d == 0, torch.zeros_like(d), d / r.bound)
    return float(q.max())


def assert_within(got, r, label):
    assert tuple(got.shape) == tuple(r.ref.shape), (label, tuple(got.shape), tuple(r.ref.shape))
    q = ratio(got, r)
    print("%s: max |d| / bound = %.3f" % (label, q))
    assert q <= 1.0, (label, q)
    return q


# ---- InstanceNorm, separate statistics pass (in_stats_kernel / in_finalize_kernel / in_apply_kernel) ----------------------------------------------------------------
FORMS = ("plain", "relu", "residual", "leaky")
SLOPE = 0.2


def chunk_len(hw):
    """pixels per statistics chunk (gdt_k_instance_norm): ceil(HW / ceil(HW / 1024))"""
    n = max(1, (hw + 1023) // 1024)
    return (hw + n - 1) // n


def stat_errors(x, eps=EPS_NORM):
    """(e_r, e_m) per (n, c), [N, C, 1, 1]: the relative error of rstd and the error of the mean in units of the standard deviation, for statistics the device takes
    from the STORED tensor ``x``.  in_stats_kernel adds the k pixels of a chunk (and their squares: one more rounding) in fp32 in some order, in_finalize_kernel adds
    the chunks' partial sums in fp64 (exact at this scale) and rounds mean and rstd to fp32.  With g = g_(k+1), A1 = mean |x| and A2 = mean x^2:
        sum:      |s' - s| <= g sum |x|      ->  |m' - m| <= g A1 in fp64, + u |m| stored
        squares:  |q' - q| <= g sum x^2
        variance: var' = q' / HW - m'^2      ->  |var' - var| <= g A2 + 2 |m| g A1 + (g A1)^2 = dvar
        rstd:     rstd' / rstd = sqrt((var + eps) / (var' + eps)) <= 1 / sqrt(1 - t),  t = dvar / (var + eps);  + u stored (the product of the two is < 1e-11)
    dvar / var grows with 1 + (m / std)^2: the cancellation of q / HW - m^2 is in the bound, not hidden."""
    x = x.double()
    g = gamma(chunk_len(x.shape[2] * x.shape[3]) + 1)
    m = x.mean(dim=(2, 3), keepdim=True)
    var = x.var(dim=(2, 3), unbiased=False, keepdim=True)
    a1, a2 = x.abs().mean(dim=(2, 3), keepdim=True), (x * x).mean(dim=(2, 3), keepdim=True)
    dm = g * a1 + U32 * m.abs()
    dvar = g * a2 + 2 * m.abs() * g * a1 + (g * a1) ** 2
    t = dvar / (var + eps)
    assert float(t.max()) < 0.5, float(t.max())
    return 1.0 / torch.sqrt(1 - t) - 1 + U32, dm / torch.sqrt(var + eps)


def instance_norm(x, form, residual=None, out_f32=False, slope=SLOPE, eps=EPS_NORM):
    """float64 InstanceNorm of the tapped tensor ``x`` in one of FORMS and its bound: stat_errors() per channel through the dz of conv_bound.norm_value (|z| e_r +
    e_m (1 + e_r) + the two fp32 operations of (x - mean') * rstd'; ReLU and LeakyReLU are 1-Lipschitz; a residual adds one rounding of the sum), + u |a| for the
    LeakyReLU product, then the store: 2^-11 (|a| + dz) + 2^-25 in fp16, u |a| for the fp32 tensors of f16x3"""
    e_r, e_m = stat_errors(x, eps)
    a, dz = cb.norm_value(x, relu=form == "relu", residual=residual if form == "residual" else None, eps=eps, err_r=e_r, err_m=e_m)
    if form == "leaky":
        a = torch.where(a > 0, a, a * float(np.float32(slope)))
        dz = dz + U32 * a.abs()
    return Ref(a, dz + (U32 * a.abs() if out_f32 else U16 * (a.abs() + dz) + SUB16))


def emulate_instance_norm(x, form, residual=None, out_f32=False, slope=SLOPE, fault=None):
    """what the three kernels compute, in fp32 on the CPU: conv_bound.emulate_stats per chunk (fp32 partial sums, fp64 finish), then (x - mean) * rstd, the
    activation, the residual, one store.  ``fault``: "no_mm" (variance without the m * m term), "unbiased" (HW - 1 in the variance), "skip_pixel" (the first pixel
    left out of the sums), "skip_chunk" (the last chunk left out; needs more than one chunk)"""
    x32 = x.float()
    n, c, h, w = x32.shape
    hw, k = h * w, chunk_len(h * w)
    if fault is None:
        mean, rstd = cb.emulate_stats(x32, rows=k)
    else:
        flat = x32.reshape(n, c, hw)
        if fault == "skip_pixel":
            flat = flat[:, :, 1:]
        elif fault == "skip_chunk":
            assert hw > k
            flat = flat[:, :, :(hw - 1) // k * k]
        s = torch.zeros(n, c, dtype=torch.float64)
        q = torch.zeros(n, c, dtype=torch.float64)
        for r0 in range(0, flat.shape[2], k):
            part = flat[:, :, r0:r0 + k]
            s += part.sum(dim=2, dtype=torch.float32).double()
            q += (part * part).sum(dim=2, dtype=torch.float32).double()
        mean = s / hw
        var = (q / hw - (0 if fault == "no_mm" else mean * mean)).clamp_min(0)
        if fault == "unbiased":
            var = var * hw / (hw - 1)
        mean, rstd = mean.float().double(), (1.0 / torch.sqrt(var + EPS_NORM)).float().double()
    f = (x32 - mean.float()[:, :, None, None]) * rstd.float()[:, :, None, None]
    if form == "relu":
        f = F.relu(f)
    elif form == "leaky":
        f = torch.where(f > 0, f, f * float(np.float32(slope)))
    elif form == "residual":
        f = f + residual.float()
    return f if out_f32 else cb.f16(f)


# ---- bilinear sampling at fp32 coordinates (pack_input_kernel, hed_fuse_kernel) -------------------------------------------------------------------------------------
Axis = collections.namedtuple("Axis", "i0 i1 lam ulp")


def source_axis(n_in, n_out, rscale, half_pixel=True):
    """torch's source coordinates along one axis, src = max(rscale * (dst + 0.5) - 0.5, 0), evaluated in fp32 operation by operation as aten evaluates them
    (``rscale`` an np.float32); i0 = floor(src), i1 = i0 + (i0 < in - 1), lam = src - i0 in float64.  ``ulp``: the fp32 spacing at the product rscale * (dst + 0.5),
    the one operation of the expression that rounds (the subtraction of 0.5 from it is exact) -- see bilinear()."""
    d = np.arange(n_out, dtype=np.float32)
    r = np.float32(rscale)
    prod = r * (d + np.float32(0.5)) if half_pixel else r * d
    src = np.maximum(prod - np.float32(0.5), np.float32(0)) if half_pixel else prod
    assert src.dtype == np.float32
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    return Axis(i0, i0 + (i0 < n_in - 1), src.astype(np.float64) - i0, np.spacing(prod).astype(np.float64))


def _taps(v, ay, ax):
    g = lambda yy, xx: v[:, :, yy][:, :, :, xx]
    return g(ay.i0, ax.i0), g(ay.i0, ax.i1), g(ay.i1, ax.i0), g(ay.i1, ax.i1)


def _max4(taps):
    return torch.stack([t.abs() for t in taps]).max(0).values


def bilinear(v, ay, ax, dv=None):
    """(value, error before any store) of (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11) in float64 at the coordinates of source_axis().
    * Coordinates.  The device evaluates src in fp32 as the reference does, but the compiler may contract the multiply-subtract into one fma: the two forms differ by
      the rounding of the product, at most one fp32 ulp at the product (``ulp``).  As a function of src the interpolation is continuous and piecewise linear -- also
      across an integer, where floor() flips -- with slope at most L = max |v[i + 1] - v[i]| along that axis (taken over the whole map, per image and channel): L ulp per axis.
    * Weights.  lam = src - i0 is exact; 1 - lam rounds once; allowed 2 u per axis, times m = max |tap|.
    * Arithmetic.  Three fp32 operations per tap and the final sum, weights summing to 1: <= 2 u m; allowed 8 u m as in test_hip_dynint_unet.py.
    * ``dv``: an error already on the map.  A convex combination carries at most the largest error of its four taps; L and m grow by it."""
    v = v.double()
    taps = _taps(v, ay, ax)
    ly, lx = torch.from_numpy(ay.lam)[None, None, :, None], torch.from_numpy(ax.lam)[None, None, None, :]
    ref = (1 - ly) * ((1 - lx) * taps[0] + lx * taps[1]) + ly * ((1 - lx) * taps[2] + lx * taps[3])
    m = _max4(taps)
    lip_y = (v[:, :, 1:] - v[:, :, :-1]).abs().amax(dim=(2, 3), keepdim=True) if v.shape[2] > 1 else torch.zeros_like(v[:, :, :1, :1])
    lip_x = (v[:, :, :, 1:] - v[:, :, :, :-1]).abs().amax(dim=(2, 3), keepdim=True) if v.shape[3] > 1 else torch.zeros_like(v[:, :, :1, :1])
    carried = 0.0
    if dv is not None:
        carried = _max4(_taps(dv.double(), ay, ax))
        worst = dv.double().amax(dim=(2, 3), keepdim=True)
        lip_y, lip_x, m = lip_y + 2 * worst, lip_x + 2 * worst, m + carried
    uy, ux = torch.from_numpy(ay.ulp)[None, None, :, None], torch.from_numpy(ax.ulp)[None, None, None, :]
    return ref, carried + lip_y * uy + lip_x * ux + (2 + 2 + 8) * U32 * m


def emulate_bilinear(v, oh, ow, ry, rx, half_pixel=True):
    """the kernels' interpolation in fp32 on the CPU, operation by operation (no fma); ``half_pixel`` False: the wrong kernel that leaves the half-pixel offset out"""
    def axis(n_in, n_out, r):
        d = np.arange(n_out, dtype=np.float32)
        s = np.maximum(np.float32(r) * (d + np.float32(0.5)) - np.float32(0.5), np.float32(0)) if half_pixel else np.float32(r) * d
        i0 = np.minimum(s.astype(np.int64), n_in - 1)
        l1 = (s - i0.astype(np.float32)).astype(np.float32)
        return i0, i0 + (i0 < n_in - 1), torch.from_numpy(l1), torch.from_numpy(np.float32(1) - l1)
    v = v.float()
    y0, y1, ly1, ly0 = axis(v.shape[2], oh, ry)
    x0, x1, lx1, lx0 = axis(v.shape[3], ow, rx)
    g = lambda yy, xx: v[:, :, yy][:, :, :, xx]
    ly1, ly0, lx1, lx0 = ly1[None, None, :, None], ly0[None, None, :, None], lx1[None, None, None, :], lx0[None, None, None, :]
    return ly0 * (lx0 * g(y0, x0) + lx1 * g(y0, x1)) + ly1 * (lx0 * g(y1, x0) + lx1 * g(y1, x1))


def resized_size(h, w, scale):
    """F.interpolate(scale_factor=s): floor(float(in * s))"""
    return int(math.floor(float(h * scale))), int(math.floor(float(w * scale)))


def _affine(c, perm, scale, shift):
    perm = list(range(c)) if perm is None else list(perm)
    sc = torch.tensor([1.0] * c if scale is None else scale, dtype=torch.float32).double().view(1, -1, 1, 1)
    sh = torch.tensor([0.0] * c if shift is None else shift, dtype=torch.float32).double().view(1, -1, 1, 1)
    return perm, sc, sh


def pack_input(x, scale_factor, out_f32, perm=None, scale=None, shift=None):
    """the input op with a resize: F.interpolate(x[:, perm], scale_factor=s, bilinear, align_corners=False) * scale + shift.  rscale = fp32(1 / s) as the engine
    passes it.  Bound: bilinear() times |scale|; with an affine its product and its sum round once each (u |v scale| + u |ref|; an fma rounds less); then the fp16
    store 2^-11 (|ref| + e) + 2^-25.  The fp32 tensor of f16x3 holds the fp32 result as it is: no further term."""
    perm, sc, sh = _affine(x.shape[1], perm, scale, shift)
    oh, ow = resized_size(x.shape[2], x.shape[3], scale_factor)
    r = np.float32(1.0 / scale_factor)
    v, e = bilinear(x[:, perm], source_axis(x.shape[2], oh, r), source_axis(x.shape[3], ow, r))
    ref = v * sc + sh
    e = e * sc.abs()
    if scale is not None or shift is not None:
        e = e + U32 * ((v * sc).abs() + ref.abs())
    return Ref(ref, e if out_f32 else e + U16 * (ref.abs() + e) + SUB16)


def emulate_pack_input(x, scale_factor, out_f32, perm=None, scale=None, shift=None, half_pixel=True):
    perm, sc, sh = _affine(x.shape[1], perm, scale, shift)
    oh, ow = resized_size(x.shape[2], x.shape[3], scale_factor)
    r = np.float32(1.0 / scale_factor)
    o = emulate_bilinear(x[:, perm], oh, ow, r, r, half_pixel) * sc.float() + sh.float()
    return o if out_f32 else cb.f16(o)


# ---- HED head (hed_score_kernel / hed_fuse_kernel) -------------------------------------------------------------------------------------------------------------------
def hed_head(feats, score_w, score_b, fusion_w, fusion_b, size):
    """float64 pre-sigmoid output of the HED head on the five tapped maps and its bound.
    * Score s_k = b_k + sum_c x_c w_c with fp32 weights: C products that round, C additions in some order (8 lanes, a butterfly, the bias):
      |ds_k| <= g_(C+1) (sum |x| |w| + |b|).
    * Upsampling to ``size``: bilinear() with rscale = fp32(h) / fp32(H) as torch and the kernel take it, ds_k carried by the taps: e_k.
    * Fusion fb + sum_k fw_k v_k: five products and five additions, |d| <= sum |fw_k| e_k + g_6 (sum |fw_k v_k| + |fb|)."""
    H, W = size
    pre, mag, err = float(np.float32(fusion_b)), abs(float(np.float32(fusion_b))), 0.0
    for x, w, b, fw in zip(feats, score_w, score_b, fusion_w):
        x = x.double()
        w64 = w.reshape(-1).float().double()[None, :, None, None]
        b64, fw64 = float(np.float32(b)), float(np.float32(fw))
        s = (x * w64).sum(1, keepdim=True) + b64
        ds = gamma(x.shape[1] + 1) * ((x.abs() * w64.abs()).sum(1, keepdim=True) + abs(b64))
        h, wd = x.shape[2:]
        v, e = bilinear(s, source_axis(h, H, np.float32(h) / np.float32(H)), source_axis(wd, W, np.float32(wd) / np.float32(W)), dv=ds)
        pre, mag, err = pre + fw64 * v, mag + (fw64 * v).abs(), err + abs(fw64) * e
    return Ref(pre, err + gamma(6) * mag)


def hed_sigmoid(pre, sigmoid_u):
    """sigmoid(pre) and its bound: |sigmoid'| <= 1 / 4 carries the pre-sigmoid bound, and the device's 1 / (1 + expf(-v)) is allowed ``sigmoid_u`` u of its result"""
    ref = torch.sigmoid(pre.ref)
    return Ref(ref, pre.bound / 4 + sigmoid_u * U32 * ref)


# ---- GeM + L2N (gem_kernel / l2n_rows_kernel) ------------------------------------------------------------------------------------------------------------------------
def gem_l2n(x, p, eps_gem=EPS_POOL, eps_l2=EPS_POOL):
    """float64 (mean_px clamp(x, eps)^p)^(1 / p), then v / (||v|| + eps), on the tapped map ``x`` [N, D, H, W], and its bound.  p and 1 / p are the fp32 numbers the
    kernel holds: p32 = fp32(p), q32 = 1.0f / p32.
    * One term clamp(x, eps)^p: f * f * f rounds twice (p = 3), powf is within 16 ulp otherwise: relative tau = g_2 or 16 * 2^-23.
    * The sum of HW terms in any order, g_HW, and the division by HW, u: the mean is M' = M (1 + d), 1 + |d| <= (1 + tau)(1 + g_HW)(1 + u).
    * pooled' = powf(M', q32) = M^(1/p32) (1 + d)^q32 M^(q32 - 1/p32) (1 + 16 ulp): in logarithms
          |ln(pooled' / pooled)| <= q32 |ln(1 - |d|)| + |ln M| |q32 - 1 / p32| + |ln(1 - 16 ulp)| = ln(1 + rel_c)
      -- the term error divided by p, the rounding of 1 / p scaled by |ln mean| (|q32 p32 - 1| is computed, not bounded: 0 for p = 1), the outer powf.
    * Norm: s' = sum v'^2 with D products and D additions in some order, sqrtf, + eps, each correctly rounded.  sqrt(sum v_c^2 (1 + rel_c)^2) / ||v|| - 1 = R is
      what the channels' own errors do to the norm; the denominator is off by at most E = (1 + R)(1 + g_(D+1))(1 + u)^2 - 1 (the whole g, not its half: any order).
    * The final division rounds once: |y' / y - 1| <= (1 + rel_c)(1 + u) / (1 - E) - 1.  Everything is relative to |y|."""
    p32 = float(np.float32(p))
    q32 = float(np.float32(1.0) / np.float32(p))
    x = x.double()
    n, d, h, w = x.shape
    hw = h * w
    mean = (x.clamp_min(eps_gem) ** p32).mean(dim=(2, 3))
    pooled = mean ** (1.0 / p32)
    norm = pooled.norm(dim=1, keepdim=True)
    ref = pooled / (norm + eps_l2)
    tau = gamma(2) if p32 == 3.0 else POWF_ULPS * 2 * U32
    dl = (1 + tau) * (1 + gamma(hw)) * (1 + U32) - 1
    rel = torch.expm1(-q32 * math.log1p(-dl) + mean.log().abs() * abs(q32 * p32 - 1) / p32 - math.log1p(-POWF_ULPS * 2 * U32))
    R = (pooled * (1 + rel)).norm(dim=1, keepdim=True) / norm - 1
    E = (1 + R) * (1 + gamma(d + 1)) * (1 + U32) ** 2 - 1
    return Ref(ref, ref.abs() * ((1 + rel) * (1 + U32) / (1 - E) - 1))


def emulate_gem_l2n(x, p, eps_gem=EPS_POOL, eps_l2=EPS_POOL, fault=None):
    """the two kernels in fp32 on the CPU.  ``fault``: "no_clamp" (x^p of the raw values), "skip_tail" (the pixels past the last full group of 32 left out of the sum)"""
    p32 = np.float32(p)
    x = x.float()
    n, d, h, w = x.shape
    flat = x.reshape(n, d, h * w)
    if fault == "skip_tail":
        flat = flat[:, :, :h * w // 32 * 32]
    f = flat if fault == "no_clamp" else flat.clamp_min(float(np.float32(eps_gem)))
    t = f * f * f if float(p32) == 3.0 else torch.pow(f, float(p32))
    pooled = torch.pow(t.sum(dim=2, dtype=torch.float32) / np.float32(h * w), float(np.float32(1.0) / p32))
    nrm = torch.sqrt((pooled * pooled).sum(dim=1, keepdim=True, dtype=torch.float32)) + float(np.float32(eps_l2))
    return pooled / nrm


# ---- the cases both test files run -------------------------------------------------------------------------------------------------------------------------------------
# InstanceNorm: (norm input shape (N, C, H, W), std of the producing conv's bias); every H W is no multiple of 128, so no producer delivers fused statistics
INORM_CASES = [((2, 32, 24, 40), 0.5),      # 960 pixels: one chunk
               ((2, 8, 25, 41), 0.5),       # 1025: two chunks of 513; C / 8 = 1, 256 pixel rows per workgroup
               ((1, 256, 45, 47), 0.5),     # 2115: three chunks of 705, the last one ragged; 8 pixel rows
               ((2, 1024, 3, 5), 0.5),      # 15: 2 pixel rows, most of them idle
               ((1, 64, 33, 31), 0.5),      # 1023: just under one chunk
               ((2, 32, 24, 40), 1.5)]      # |mean| / std up to about 6
SQRT2 = math.sqrt(2.0)
# input pack: (image shape, scale_factor, (perm, scale, shift) or None)
PACK_CASES = [((2, 3, 40, 56), 1 / SQRT2, None), ((2, 3, 40, 56), 0.5, None), ((2, 3, 40, 56), SQRT2, None), ((2, 3, 40, 56), 0.3, None), ((2, 3, 40, 56), 1.9, None),
              ((1, 3, 37, 53), 1 / SQRT2, None), ((2, 1, 37, 53), 0.5, None),
              ((2, 3, 40, 56), 1 / SQRT2, ([2, 1, 0], [0.5, 2.0, 1.0], [0.1, -0.2, 0.3]))]
# GeM: (D, (H, W), p, ReLU on the producing conv): 30, 77 and 1023 pixels; without the ReLU the map has negative values and the clamp matters
GEM_CASES = [(64, (5, 6), 3.0, True), (64, (7, 11), 2.37, False), (64, (33, 31), 1.0, False), (512, (5, 6), 2.37, True), (512, (33, 31), 3.0, False),
             (2048, (7, 11), 1.0, True), (2048, (33, 31), 2.37, True), (2048, (5, 6), 3.0, False)]


def case_id(case):
    part = lambda v: "affine" if isinstance(v, tuple) and isinstance(v[0], list) else "x".join(str(e) for e in v) if isinstance(v, tuple) else \
        "%.3g" % v if isinstance(v, float) else str(v)
    return "-".join(part(v) for v in case if v is not None)


def conv1x1_cpu(x, w, b, out_f32, relu=False):
    """a stand-in for the producing 1 x 1 conv on the CPU: the tensor an op under test consumes, fp16 numbers unless ``out_f32``"""
    y = F.conv2d(x.float(), w.float(), b)
    y = F.relu(y) if relu else y
    return y if out_f32 else cb.f16(y)
