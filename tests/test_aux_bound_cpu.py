"""The bounds of aux_bound.py checked without a GPU: an fp32 emulation of a correct kernel stays within each bound on every case of test_hip_aux_ops.py, and the wrong
kernels the older global gates let through exceed it on every case where they apply.  The ratios are printed (pytest -s)."""
import numpy as np
import pytest
import torch

import aux_bound as ab
from gandtr_amd.tools import synth


# ---- InstanceNorm ------------------------------------------------------------------------------------------------------------------------------------------------------
def _inorm_tensors(case, out_f32):
    (n, c, h, w), bias_std = case
    x = synth.synth_input(11, (n, 3, h, w))
    a = ab.conv1x1_cpu(x, synth._normal(11, "wa", (c, 3, 1, 1), 0.7), synth._normal(11, "ba", (c,), bias_std), out_f32)
    b = ab.conv1x1_cpu(x, synth._normal(11, "wb", (c, 3, 1, 1), 0.7), None, out_f32)
    return a, b


@pytest.mark.parametrize("out_f32", [False, True], ids=["f16", "f32"])
@pytest.mark.parametrize("case", ab.INORM_CASES, ids=ab.case_id)
def test_instance_norm_bound_holds_a_correct_kernel_and_no_wrong_one(case, out_f32):
    """correct: <= 1 in every form.  Variance without m * m, the unbiased variance, one pixel left out of the sums, the last chunk left out (where there is more than
    one): > 1 in every form.  Measured here: correct 0.84 - 0.99 (fp16: the half ulp of the store) and 0.002 - 0.19 (fp32); wrong: no m * m >= 320, one pixel left
    out >= 23, last chunk left out >= 7000, and the smallest of all, the unbiased variance on 2115 pixels, 1.37 (fp16) and 7.8 (fp32)."""
    a, b = _inorm_tensors(case, out_f32)
    hw = a.shape[2] * a.shape[3]
    faults = ["no_mm", "unbiased", "skip_pixel"] + (["skip_chunk"] if hw > ab.chunk_len(hw) else [])
    ratios = a.double().mean(dim=(2, 3)).abs() / a.double().std(dim=(2, 3), unbiased=False)
    print("%s %s: |mean| / std up to %.2f" % (ab.case_id(case), "f32" if out_f32 else "f16", float(ratios.max())))
    for form in ab.FORMS:
        r = ab.instance_norm(a, form, residual=b, out_f32=out_f32)
        q = ab.ratio(ab.emulate_instance_norm(a, form, residual=b, out_f32=out_f32), r)
        wrong = {f: ab.ratio(ab.emulate_instance_norm(a, form, residual=b, out_f32=out_f32, fault=f), r) for f in faults}
        print("  %-8s correct %.3f   %s" % (form, q, "   ".join("%s %.3g" % kv for kv in wrong.items())))
        assert q <= 1.0, (form, q)
        for f, v in wrong.items():
            assert v > 1.0, (form, f, v)


def test_instance_norm_bound_scales_with_the_mean_to_std_ratio():
    """the statistics term of the bound carries the cancellation of q / HW - m^2: e_r = g (A2 + ..) / var grows like 1 + (m / std)^2 (3.3e-5 at ratio 0, 3.5e-3 at
    ratio 6 on 1023 pixels: a worst case over all summation orders, so channels far beyond a biased conv's ratios are bounded loosely, by design)"""
    x = synth.synth_input(12, (1, 8, 33, 31))
    e0, _ = ab.stat_errors(x)
    e6, _ = ab.stat_errors(x + 6.0)
    print("e_r at |mean| / std ~ 0: %.2e; at ~ 6: %.2e" % (float(e0.max()), float(e6.max())))
    assert 50 * float(e0.max()) < float(e6.max()) < (1 + 3 * 6.5 ** 2) * float(e0.max())      # A2 + 2 |m| A1 ~ var (1 + 3 (m / std)^2)


# ---- input pack with resize --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_f32", [False, True], ids=["f16", "f32"])
@pytest.mark.parametrize("case", ab.PACK_CASES, ids=ab.case_id)
def test_pack_resize_bound(case, out_f32):
    """correct (the kernel's fp32 operations, not contracted): <= 1; torch's own fp32 F.interpolate: <= 1; the resize without the half-pixel offset: > 1"""
    shape, s, affine = case
    kw = dict(zip(("perm", "scale", "shift"), affine)) if affine else {}
    x = synth.synth_input(5, shape)
    r = ab.pack_input(x, s, out_f32, **kw)
    q = ab.ratio(ab.emulate_pack_input(x, s, out_f32, **kw), r)
    wrong = ab.ratio(ab.emulate_pack_input(x, s, out_f32, half_pixel=False, **kw), r)
    print("%s %s: correct %.3f, no half-pixel offset %.3g" % (ab.case_id(case), "f32" if out_f32 else "f16", q, wrong))
    assert q <= 1.0 and wrong > 1.0
    if not affine:
        t = torch.nn.functional.interpolate(x, scale_factor=s, mode="bilinear", align_corners=False)
        qt = ab.ratio(t if out_f32 else t.half().float(), r)
        print("  torch's fp32 interpolate: %.3f" % qt)
        assert qt <= 1.0


# ---- HED head: the interpolation term at the five ratios of a floor-pooled pyramid -----------------------------------------------------------------------------------
def test_hed_upsampling_term_holds_torch_interpolate():
    """maps 37x53, 18x26, 9x13, 4x6, 2x3 to 37x53 and 33x17's pyramid to 33x17: torch's fp32 F.interpolate(size=..) within the interpolation term alone"""
    for H, W in [(37, 53), (33, 17)]:
        h, w = H, W
        for k in range(5):
            v = synth.synth_input(20 + k, (2, 1, h, w))
            ref, e = ab.bilinear(v, ab.source_axis(h, H, np.float32(h) / np.float32(H)), ab.source_axis(w, W, np.float32(w) / np.float32(W)))
            got = torch.nn.functional.interpolate(v, size=(H, W), mode="bilinear", align_corners=False)
            q = ab.ratio(got, ab.Ref(ref, e))
            print("%dx%d -> %dx%d: %.3f" % (h, w, H, W, q))
            assert q <= 1.0
            h, w = h // 2, w // 2


# ---- GeM + L2N -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_f32", [False, True], ids=["f16", "f32"])
@pytest.mark.parametrize("case", ab.GEM_CASES, ids=ab.case_id)
def test_gem_l2n_bound(case, out_f32):
    """correct: <= 1.  Without the clamp: > 1 wherever the map has negative values (the conv without ReLU).  Without the pixels past the last full group of 32
    (30 -> 0, 77 -> 64, 1023 -> 992 pixels): > 1 everywhere."""
    d, (h, w), p, relu = case
    x = synth.synth_input(7, (2, 3, h, w))
    m = ab.conv1x1_cpu(x, synth._normal(7, "w", (d, 3, 1, 1), 0.7), synth._normal(7, "b", (d,), 0.5), out_f32, relu=relu)
    r = ab.gem_l2n(m, p)
    q = ab.ratio(ab.emulate_gem_l2n(m, p), r)
    tail = ab.ratio(ab.emulate_gem_l2n(m, p, fault="skip_tail"), r)
    print("%s %s: correct %.3f, tail skipped %.3g" % (ab.case_id(case), "f32" if out_f32 else "f16", q, tail))
    assert q <= 1.0 and tail > 1.0
    if not relu:
        raw = ab.ratio(ab.emulate_gem_l2n(m, p, fault="no_clamp"), r)
        print("  no clamp %.3g" % raw)
        assert raw > 1.0
