"""The bounds of blur_bound.py checked without a GPU, on every case of test_hip_blur_resample.py: an fp32 emulation of the correct op (blur_ref.emulate, the kernel's
own order of operations) stays within the bound, and each emulated wrong kernel exceeds it.  The ratios max |d| / bound are printed (pytest -s).

The inputs are what the device test feeds: a 1 x 1 conv with a bias of standard deviation 1 on N(0, 1) images, so that every channel has its own offset (a padding
mistake then shows as a step at the border, whatever the sign pattern) and every image its own statistics."""
import pytest
import torch

import aux_bound as ab
import blur_bound as bb
import blur_ref as br

CASES = br.cases()


def _tensor(shape, out_f32):
    w, b = br.producer_weights(shape[1])
    return ab.conv1x1_cpu(br.producer_input(shape), w, b, out_f32)


def _applies(fault, shape, up):
    """a wrong kernel that is the SAME function as the right one on this shape is no case: the window one pixel late weighs the two pixels of a 2-pixel axis 1/2, 1/2
    like the right one (reflection on both sides), so it needs an axis of 3; exchanged or reflected phases need an axis of 2 to differ"""
    h, w = shape[2:]
    if fault == "parity":
        return max(h, w) >= 3
    return True


def test_the_float64_ops_are_the_layers():
    """blur_ref.blur against the host mirror's modules (validated against the reference's fixtures in test_antialias_host.py) and, for the up op, against
    F.interpolate(scale_factor=2, bilinear, align_corners=False), in float64: the index tables are the layers"""
    from gandtr_amd.components.model.network import p2p_networks as P
    for shape, up in CASES:
        x = _tensor(shape, True).double()
        layer = (P.Upsample if up else P.Downsample)(shape[1]).double()
        d = float((br.blur(x, up) - layer(x)).abs().max())
        print("%s: |blur_ref - module| = %.2e" % (br.case_id((shape, up)), d))
        assert d < 1e-14
        if up:
            assert float((br.blur(x, up) - torch.nn.functional.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)).abs().max()) < 1e-14


@pytest.mark.parametrize("out_f32", [False, True], ids=["f16", "f32"])
@pytest.mark.parametrize("case", CASES, ids=br.case_id)
def test_bound_holds_the_correct_op_and_no_wrong_one(case, out_f32):
    """correct: <= 1 in the plain form and in both folded forms, with either derivation of the statistics' error.  Wrong kernels: > 1 wherever they are another
    function (see _applies).

    Measured here: correct up to 0.999 with fp16 tensors (the half ulp of the store; up to 0.384 under the looser epilogue-statistics bound), up to 0.384 with fp32
    tensors.  Wrong kernels, smallest ratio over all cases and forms, in the order zero padding, replicate for reflect (down), reflect for replicate (up), phases
    exchanged, window one pixel late, ReLU behind the blur, neighbouring statistics:
        fp16 tensors, statistics of the stored tensor   810   1650   1910   4080   5780   1630    440
        fp16 tensors, epilogue-statistics bound         261    303    200    748    229    240     77
        fp32 tensors                                   5550   4940  10800  30000  12800   8070   1130"""
    shape, up = case
    x = _tensor(shape, out_f32)
    faults = br.FAULTS_UP if up else br.FAULTS_DOWN
    for norm in br.NORMS:
        for fused in ([False] if norm is None else [False, True]):
            r = bb.blur(x, up, norm, out_f32, fused=fused)
            q = bb.ratio(br.emulate(x, up, norm, out_f32), r)
            names = [f for f in faults if _applies(f, shape, up)]
            if norm is not None:
                names += [f for f in br.FAULTS_NORM if f != "relu_after" or norm == "relu"]
            wrong = {f: bb.ratio(br.emulate(x, up, norm, out_f32, fault=f), r) for f in names}
            print("%s %s %-5s %s: correct %.3f   %s" % (br.case_id(case), "f32" if out_f32 else "f16", norm, "epilogue stats" if fused else "stored stats  ", q,
                                                       "   ".join("%s %.3g" % kv for kv in wrong.items())))
            assert q <= 1.0, (norm, fused, q)
            for f, v in wrong.items():
                assert v > 1.0, (norm, fused, f, v)


def test_a_late_window_is_the_same_function_on_two_pixels():
    """why _applies leaves the parity fault out at 2 x 2: on an axis of two pixels both windows are (x0 + x1) / 2"""
    x = _tensor((2, 8, 2, 2), True).double()
    late = br.apply_axes(x, br.down_axis(2, parity=1), br.down_axis(2, parity=1))
    assert float((br.blur(x, False) - late).abs().max()) < 1e-15
