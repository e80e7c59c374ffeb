"""Shared by test_conv_bound_cpu.py and the GPU layer tests: a float64 reference of one f16 conv layer and a derived bound per output element (no test in here).

Model of a correct kernel.  Inputs ``a`` and packed weights ``w`` are fp16 numbers, so every product a * w is exact in fp32 (11 + 11 significant bits).  The kernel adds
K products and the folded shift in fp32 in some order, applies the activation in fp32 and stores fp16 once.  With u = 2^-24 (fp32 unit round-off) and any order of
the K additions,

    |acc - pre| <= g_K (sum |a| |w| + |shift|) = g_K mag,   g_K = K u / (1 - K u)              (K = products per output; g_K = K u to first order, K u <= 6e-4)

ReLU and LeakyReLU are 1-Lipschitz, so the activation does not enlarge this; the LeakyReLU product v * slope rounds once more (u |ref|).  The fp16 store adds half an
ulp of the STORED value, at most 2^-11 (|ref| + the error before the store), or half the subnormal spacing, 2^-25, whichever is larger.  Hence

    bound = e + 2^-11 (|ref| + e) + 2^-25,   e = g_K mag          (+ 2^-24 |ref| in e with LeakyReLU)

which is K 2^-24 mag + 2^-11 |ref| with its second-order terms kept (they are 1e-6 .. 6e-4 of the first-order ones).  Where K is small (the 1 x 1 convs at Cin 16 / 32 of
test_hip_layer_bounds.py, the image stems) the bound is almost only the half ulp of the store, which a correct kernel reaches whenever |ref| is just above a power of
two: ratios of 0.99 - 1.00 there are the rounding itself, and no summation order can take a correct kernel past 1.

Further terms, each from the kernel's own arithmetic:

* Residual (``residual``).  conv_epilogue.h and conv_igemm_rb.hip both round the conv result to fp16 FIRST (the LDS transpose holds halves), then add the fp16 residual in
  fp32, apply ReLU and round again.  So one more rounding, of the pre-residual value: + 2^-11 |pre|, and the fp32 sum of two halves rounds by at most 2^-24 |pre + res|.
  The final store is the 2^-11 |ref| above (ReLU after the sum is 1-Lipschitz).
* tanh head with fp32 output (``act="tanh", out_f32=True``: conv_head7.hip).  No fp16 store, so no 2^-11 |ref| and no 2^-25.  |tanh'| <= 1 carries the accumulation
  error through unchanged; the kernel calls tanhf, which the HIP math library specifies to 2 ulp of fp32: + 2 * 2^-23 |ref|.  Seven row partials are summed in the
  combine: they are part of the K products' additions.
* Max pool 2x2 (``pool=True``).  |max_i x_i - max_i y_i| <= max_i |x_i - y_i|: the bound of a pooled element is the maximum of its window's four bounds.
* Folded InstanceNorm on the input (``norm_input``).  The kernel consumes fp16(fl32(x * rstd' - mean' * rstd')) (+ ReLU, + residual before the rounding) with (mean', rstd')
  from fp32 partial sums finished in fp64; the reference uses z = (x - mean) * rstd in float64 from the tapped fp16 tensor x, unrounded.  With e_r = |rstd' / rstd - 1| and
  e_m = |mean' - mean| * rstd,
      |z' - z| <= |z| e_r + e_m (1 + e_r) + 2 * 2^-24 (|x| + |mean|) rstd        (statistics, then the two fp32 operations)
  ReLU is 1-Lipschitz; a residual adds one fp32 rounding 2^-24 |z + res|; then the fp16 rounding 2^-11 |a| of the value staged.  This |da| per input element goes through
  the convolution as sum |da| |w| and is added to the bound; the accumulation term uses mag from the reference input, enlarged by the same sum |da| |w|.
  e_r and e_m cannot be derived without assumptions on the data: where the statistics come from a conv epilogue they are taken from the fp32 values BEFORE the fp16 store,
  so they differ from the tapped tensor's by the average of H W rounding errors.  MEASURED (emulation of both statistics paths on the shapes of the GPU tests, fp32 partial
  sums per 128 rows / per chunk, against float64 statistics of the fp16 tensor): e_r <= 1.91e-5, e_m <= 1.21e-5 (largest over all (n, c) of all shapes).  ALLOWED: twice
  that, STAT_ERR_R = 3.8e-5, STAT_ERR_M = 2.4e-5, for run-to-run data differences.  On the device the written-back tensor of the write-back modes is held to this |da|
  directly (test_hip_layer_bounds.py prints that ratio; tests/test_conv_bound_cpu.py::test_statistics_error_is_the_measured_one recomputes e_r and e_m).  They add ~1e-4 relative to the input, against 4.9e-4 of its fp16 rounding.
"""
import collections

import numpy as np
import torch
import torch.nn.functional as F

U32, U16, SUB16 = 2.0 ** -24, 2.0 ** -11, 2.0 ** -25
TANHF_ULPS = 2.0                       # HIP math library: tanhf within 2 ulp
STAT_ERR_R, STAT_ERR_M = 3.8e-5, 2.4e-5  # see the docstring: measured 1.91e-5 / 1.21e-5, times two

LayerRef = collections.namedtuple("LayerRef", "ref bound pre mag K")


def f16(t):
    return t.half().float()


def affine_f16(x, perm, scale, shift):
    """(a, da): the input op's transform as the stem loaders apply it to the fp32 image, fp16(x * scale + shift).  The C expression leaves the compiler three faithful
    forms: the exact x * scale + shift rounded ONCE to fp16, the fp32 fma rounded again to fp16 (what the input pack kernel's output equals bit for bit), or product
    and sum rounded separately.  They differ only where the fp32 result sits on an fp16 rounding tie: about one element in 10^4.  Observed on an MI355X, not
    specified anywhere: conv_stem_pair_kernel (compiled to v_fma_mix instructions) agrees with the first form at those elements.  ``a`` is the first form (float64 holds
    x * scale + shift of fp32 numbers exactly up to its own 2^-53; numpy rounds float64 to fp16 once), ``da`` the largest distance to the other two: zero except at the
    ties, an in_delta for layer(), so that a kernel in any of the three forms is held to the same bound everywhere else."""
    xp = x[:, perm].float()
    sc = torch.tensor(scale, dtype=torch.float32).view(1, -1, 1, 1)
    sh = torch.tensor(shift, dtype=torch.float32).view(1, -1, 1, 1)
    exact = xp.double() * sc.double() + sh.double()
    once = torch.from_numpy(exact.numpy().astype(np.float16).astype(np.float32))
    fma = exact.float().half().float()
    two = (xp * sc + sh).half().float()
    return once, torch.maximum((once - fma).abs(), (once - two).abs()).double()


def fold(weight, bias, bn=None, transposed=False, eps=1e-5):
    """(weights as the builder packs them, float64 of fp16 numbers, in the caller's layout; folded shift, float64 of fp32 numbers): BatchNorm folded in fp32
    (scale = g / sqrt(v + eps), shift = beta + (bias - mean) * scale, w * scale), then rounded to fp16 (net_build.hip)"""
    w = weight.detach().numpy().astype(np.float32)
    cout = w.shape[1] if transposed else w.shape[0]
    b = bias.detach().numpy().astype(np.float32) if bias is not None else np.zeros(cout, np.float32)
    if bn is not None:
        g, be, m, v = (t.detach().numpy().astype(np.float32) for t in bn)
        s = (g / np.sqrt(v + np.float32(eps))).astype(np.float32)
        shift = (be + (b - m) * s).astype(np.float32)
        w = (w * (s[None, :, None, None] if transposed else s[:, None, None, None])).astype(np.float32)
    else:
        shift = b
    return torch.from_numpy(w).half().double(), torch.from_numpy(shift).double()


def _conv64(a, w, stride, pad, reflect, dilation, transposed):
    if transposed:
        return F.conv_transpose2d(a, w, None, stride=2, padding=1, output_padding=1)
    if reflect and pad:
        a, pad = F.pad(a, (pad,) * 4, mode="reflect"), 0
    return F.conv2d(a, w, None, stride=stride, padding=pad, dilation=dilation)


def products(w, transposed=False):
    """K: the largest number of products one output sums (a k3 s2 transposed conv reads at most 2 x 2 taps per output)"""
    if transposed:
        return 4 * w.shape[0]
    return w.shape[1] * w.shape[2] * w.shape[3]


def norm_value(x, relu=False, residual=None, eps=1e-5, err_r=STAT_ERR_R, err_m=STAT_ERR_M):
    """(a, dz): norm_input's float64 value and its error BEFORE the rounding of the store; ``err_r`` / ``err_m`` are numbers or tensors that broadcast against
    [N, C, 1, 1] (aux_bound.py derives them per channel for the separate statistics pass)"""
    x = x.double()
    mean = x.mean(dim=(2, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(x.var(dim=(2, 3), unbiased=False, keepdim=True) + eps)
    z = (x - mean) * rstd
    dz = z.abs() * err_r + err_m * (1 + err_r) + 2 * U32 * (x.abs() + mean.abs()) * rstd
    a = F.relu(z) if relu else z
    if residual is not None:
        a = a + residual.double()
        dz = dz + U32 * a.abs()
    return a, dz


def norm_input(x, relu=False, residual=None, eps=1e-5, err_r=STAT_ERR_R, err_m=STAT_ERR_M):
    """(a, da): the float64 input InstanceNorm(x) (+ ReLU, + residual) of a conv that folds the norm into its staging, and the bound on what the kernel stages instead
    (see the docstring); ``x`` the tapped fp16 tensor"""
    a, dz = norm_value(x, relu, residual, eps, err_r, err_m)
    return a, dz + U16 * a.abs() + SUB16


def layer(a, w, shift, stride=1, pad=0, reflect=False, dilation=1, transposed=False, act=None, leaky=0.0, residual=None, pool=False, out_f32=False, in_delta=None):
    """float64 reference and per-output bound of one layer: ``a`` the input the layer consumed (fp16 numbers; with a folded norm the ``a`` of norm_input and its ``da``
    as ``in_delta``), ``w`` / ``shift`` from fold(); ``act`` None, "relu", "leaky" (slope ``leaky``) or "tanh"; ``residual`` an fp16 tensor added before the ReLU;
    ``pool`` a following MaxPool2d(2, 2)"""
    a, w, shift = a.double(), w.double(), shift.double()
    K = products(w, transposed)
    sh = shift[None, :, None, None]
    pre = _conv64(a, w, stride, pad, reflect, dilation, transposed) + sh
    mag = _conv64(a.abs(), w.abs(), stride, pad, reflect, dilation, transposed) + sh.abs()
    extra = torch.zeros_like(pre)
    if in_delta is not None:
        extra = _conv64(in_delta.double(), w.abs(), stride, pad, reflect, dilation, transposed)
        mag = mag + extra
    bound = K * U32 / (1 - K * U32) * mag + extra
    y = pre
    if residual is not None:
        y = pre + residual.double()
        bound = bound + U16 * (pre.abs() + bound) + SUB16 + U32 * y.abs()
    if act == "relu":
        ref = F.relu(y)
    elif act == "leaky":
        ref = torch.where(y > 0, y, y * float(np.float32(leaky)))
        bound = bound + U32 * ref.abs()
    elif act == "tanh":
        ref = torch.tanh(y)
        bound = bound + TANHF_ULPS * 2.0 ** -23 * ref.abs()
    else:
        assert act is None, act
        ref = y
    if not out_f32:
        bound = bound + U16 * (ref.abs() + bound) + SUB16
    if pool:
        ref, bound = F.max_pool2d(ref, 2, 2), F.max_pool2d(bound, 2, 2)
    return LayerRef(ref, bound, pre, mag, K)


def ratio(got, r):
    """(max |d| / bound, its position (n, c, y, x), max |d| / max |ref| -- the figure of the global gate this bound replaces)"""
    d = (got.double() - r.ref).abs()
    q = d / r.bound
    pos = np.unravel_index(int(torch.argmax(q)), tuple(q.shape))
    return float(q.max()), tuple(int(p) for p in pos), float(d.max() / r.ref.abs().max().clamp_min(1e-300))


def assert_within(got, r, label):
    """every output within its bound; prints max |d| / bound, where it is, and the old global figure"""
    assert tuple(got.shape) == tuple(r.ref.shape), (label, tuple(got.shape), tuple(r.ref.shape))
    assert bool(torch.isfinite(got).all()), label
    q, pos, rel = ratio(got, r)
    print("%s: max |d| / bound = %.3f at (n, c, y, x) = %s of %s; max|d| / max|ref| = %.2e" % (label, q, pos, tuple(got.shape), rel))
    assert q <= 1.0, (label, q, pos)
    return q


def assert_layer(got, a, w, shift, label, images=None, in_delta=None, residual=None, **kw):
    """assert_within image by image (the float64 tensors of a whole batch need not exist at once) over ``images`` (default: all): ``a``, ``in_delta`` and ``residual`` are
    batches, ``kw`` goes to layer(); prints and returns the largest ratio"""
    assert bool(torch.isfinite(got).all()), label
    worst = (-1.0, None, 0.0)
    for n in (range(got.shape[0]) if images is None else images):
        sl = slice(n, n + 1)
        r = layer(a[sl], w, shift, in_delta=None if in_delta is None else in_delta[sl], residual=None if residual is None else residual[sl], **kw)
        assert tuple(got[sl].shape) == tuple(r.ref.shape), (label, tuple(got.shape), tuple(r.ref.shape))
        q, pos, rel = ratio(got[sl], r)
        if q > worst[0]:
            worst = (q, (n,) + pos[1:], rel)
    print("%s: max |d| / bound = %.3f at (n, c, y, x) = %s of %s; max|d| / max|ref| of that image = %.2e" % ((label,) + worst[:2] + (tuple(got.shape), worst[2])))
    assert worst[0] <= 1.0, (label,) + worst[:2]
    return worst[0]


# ---- the emulation of a correct kernel (and of two wrong ones), on the CPU in fp32 ------------------------------------------------------------------------------------
def _columns(a, w, stride, pad, reflect, dilation):
    """im2col in tap-major order (k = (ky * kw + kx) * cin + c, the order the kernels walk K): fp32 [N, K, L] and the matching [cout, K] weights"""
    a = a.float()
    if pad:
        a = F.pad(a, (pad,) * 4, mode="reflect" if reflect else "constant")
    cout, cin, kh, kw = w.shape
    cols = F.unfold(a, (kh, kw), dilation=dilation, stride=stride)                       # [N, cin * kh * kw, L], channel-major
    n, _, L = cols.shape
    cols = cols.reshape(n, cin, kh * kw, L).permute(0, 2, 1, 3).reshape(n, kh * kw * cin, L)
    wm = w.float().reshape(cout, cin, kh * kw).permute(0, 2, 1).reshape(cout, kh * kw * cin)
    oh = (a.shape[2] - dilation * (kh - 1) - 1) // stride + 1
    return cols, wm, oh


def emulate(a, w, shift, stride=1, pad=0, reflect=False, dilation=1, transposed=False, act=None, leaky=0.0, residual=None, pool=False, out_f32=False, fault=None,
            in_stage=None):
    """what a correct kernel computes: fp32 accumulation, fp32 epilogue, one fp16 store (a residual: the two stores of conv_epilogue.h).  ``fault``: "chunk16" rounds the
    accumulator to fp16 between 64-wide K chunks, "bias_late" adds the shift after the fp16 store (a second rounding).  ``in_stage``: the fp16 tensor staged in place of ``a``
    (folded norm)."""
    x = (in_stage if in_stage is not None else a).float()
    wf, sh = w.float(), shift.float()[None, :, None, None]
    if transposed:
        assert fault is None
        acc = F.conv_transpose2d(x, wf, None, stride=2, padding=1, output_padding=1)
    elif fault == "chunk16":
        cols, wm, oh = _columns(x, w, stride, pad, reflect, dilation)
        acc = torch.zeros(cols.shape[0], wm.shape[0], cols.shape[2])
        for k0 in range(0, wm.shape[1], 64):
            acc = f16(acc + torch.matmul(wm[:, k0:k0 + 64], cols[:, k0:k0 + 64]))
        acc = acc.reshape(cols.shape[0], wm.shape[0], oh, -1)
    else:
        acc = _conv64(x, wf, stride, pad, reflect, dilation, False)
    v = f16(f16(acc) + sh) if fault == "bias_late" else acc + sh
    if residual is not None:
        v = f16(v) + residual.float()
    if act == "relu":
        v = F.relu(v)
    elif act == "leaky":
        v = torch.where(v > 0, v, v * float(np.float32(leaky)))
    elif act == "tanh":
        v = torch.tanh(v)
    if not out_f32:
        v = f16(v)
    return F.max_pool2d(v, 2, 2) if pool else v


def emulate_stats(v32, rows=128):
    """(mean', rstd') as the device takes them from fp32 values ``v32`` [N, C, H, W]: fp32 sums and sums of squares over ``rows`` pixels, finished in float64"""
    n, c = v32.shape[:2]
    flat = v32.float().reshape(n, c, -1)
    hw = flat.shape[2]
    s = torch.zeros(n, c, dtype=torch.float64)
    q = torch.zeros(n, c, dtype=torch.float64)
    for r0 in range(0, hw, rows):
        part = flat[:, :, r0:r0 + rows]
        s += part.sum(dim=2, dtype=torch.float32).double()
        q += (part * part).sum(dim=2, dtype=torch.float32).double()
    mean = s / hw
    var = (q / hw - mean * mean).clamp_min(0)
    return mean.float().double(), (1.0 / torch.sqrt(var + 1e-5)).float().double()
