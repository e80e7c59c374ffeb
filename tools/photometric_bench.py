"""dev tool: time and accuracy of the photometric launches (gandtr_amd/csrc/photometric.hip) -> profiles/photometric_1gpu.json.
usage: tools/photometric_bench.py [--out profiles/photometric_1gpu.json] [--quick]

Timing: device events around `iters` back-to-back calls (iters sized so that a window lasts about 50 ms), 5 windows per figure in this one process, reported as
median with min - max.  Shapes: 128x3x256x256 and 4x3x1024x1024, generator-like images with the (0.5, 0.5) affine pair.  Compared with clahe.clahe_lab on the same
tensor (the same pass structure at 38 B / pixel) and with the same op sequence written in torch ops on the same GPU (float32 Lab, bincount, cumsum, a searchsorted
interpolation, a batched secant of 12 fixed steps with one pow().mean() each and no host round trip -- fewer syncs than a per-image port would have).
Algorithmic bytes: 36 B / pixel for histogram matching, 44 B / pixel for gamma equalisation (pass 1 also writes the fp32 lightness plane, the solve's reads are
L2 hits at these sizes and are not counted); TB/s = those bytes over the median time, a whole-call figure, not a kernel's share of peak.
Accuracy: the lightness plane's largest ratio to its first-order bound (tests/photometric_ref.py) and the difference of the fused forms to the pure oracle pipeline
(oracle Lab -> numpy channel function -> oracle Lab back), which includes the pixels a one-ulp lightness difference moves across a bin edge."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                                            # noqa: E402
import torch                                                  # noqa: E402

from gandtr_amd import clahe, photometric                     # noqa: E402
from gandtr_amd.components.data import photometric as P       # noqa: E402

PAIR = ([0.5] * 3, [0.5] * 3)
NAME = "f3d_lab"


def images(seed, n, h, w):
    g = torch.Generator().manual_seed(seed)
    low = torch.nn.functional.interpolate(torch.randn(n, 3, 9, 9, generator=g), size=(h, w), mode="bicubic", align_corners=False)
    return torch.tanh(0.9 * low + 0.15 * torch.randn(n, 3, h, w, generator=g)).contiguous()


def timed(fn, windows=5, target_ms=50.0):
    """median / min / max milliseconds per call over `windows` event-timed windows"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        fn()
    e1.record()
    torch.cuda.synchronize()
    iters = int(min(max(target_ms / max(e0.elapsed_time(e1) / 5, 1e-3), 10), 1000))
    times = []
    for _ in range(windows):
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / iters)
    return {"ms_median": round(statistics.median(times), 5), "ms_min": round(min(times), 5), "ms_max": round(max(times), 5), "iters": iters, "windows": windows}


# ---- the same op sequence in torch ops (float32 Lab with OpenCV's constants) ----

def torch_ops(dev, cdf_name):
    fwd = torch.tensor((P._RGB2XYZ / P._WHITE[:, None]).astype(np.float32), device=dev)
    inv = torch.tensor((P._XYZ2RGB * P._WHITE[None, :]).astype(np.float32), device=dev)
    centres = torch.tensor(photometric.HISTOGRAM_CENTERS, device=dev)
    target = torch.tensor(np.cumsum(photometric._HISTOGRAMS[cdf_name]), device=dev)

    def to_lab(x):
        c = (x * 0.5 + 0.5).clamp(0, 1)
        lin = torch.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
        xyz = torch.einsum("ij,njhw->nihw", fwd, lin)
        f = torch.where(xyz > 0.008856, xyz.clamp_min(1e-30) ** (1.0 / 3.0), 7.787 * xyz + 16.0 / 116.0)
        L = torch.where(xyz[:, 1] > 0.008856, 116.0 * f[:, 1] - 16.0, 903.3 * xyz[:, 1]) / 100.0
        return L, f[:, 0] - f[:, 1], f[:, 1] - f[:, 2]

    def to_rgb(Ln, a500, b200):
        L = Ln * 100.0
        low = L <= 0.008856 * 903.3
        fy = torch.where(low, 7.787 * (L / 903.3) + 16.0 / 116.0, (L + 16.0) / 116.0)
        y = torch.where(low, L / 903.3, fy ** 3)
        fth = 7.787 * 0.008856 + 16.0 / 116.0
        fx, fz = a500 + fy, fy - b200
        xyz = torch.stack([torch.where(fx <= fth, (fx - 16.0 / 116.0) / 7.787, fx ** 3), y, torch.where(fz <= fth, (fz - 16.0 / 116.0) / 7.787, fz ** 3)], dim=1)
        c = torch.einsum("ij,njhw->nihw", inv, xyz).clamp(0, 1)
        rgb = torch.where(c <= 0.0031308, c * 12.92, 1.055 * c.clamp_min(1e-30) ** (1.0 / 2.4) - 0.055)
        return (rgb - 0.5) / 0.5

    def interp(x, xp, fp):
        j = (torch.searchsorted(xp, x.contiguous(), right=True) - 1).clamp(0, 254)
        x0, x1, f0, f1 = xp.gather(-1, j), xp.gather(-1, j + 1), fp.gather(-1, j), fp.gather(-1, j + 1)
        return torch.where(x1 > x0, f0 + (f1 - f0) / (x1 - x0).clamp_min(1e-300) * (x - x0), f0)

    def match(x, named):
        L, a, b = to_lab(x)
        n = L.shape[0]
        flat = L.reshape(n, -1).double()
        bins = (flat * 255.0 + 0.5).floor().clamp(0, 255).long() + 256 * torch.arange(n, device=dev)[:, None]
        hist = torch.bincount(bins.reshape(-1), minlength=n * 256).reshape(n, 256)
        cdf = hist.cumsum(1).double() / flat.shape[1]
        table = interp(cdf, target[None].expand(n, 256).contiguous(), centres[None].expand(n, 256).contiguous()) if named else cdf * centres[-1]
        mapped = interp(flat, centres[None].expand(n, 256).contiguous(), table.contiguous()).float().reshape(L.shape)
        return to_rgb(mapped, a, b)

    def gamma(x, t):
        L, a, b = to_lab(x)
        n = L.shape[0]
        flat = L.reshape(n, -1).double()
        f = lambda g: (flat ** g[:, None]).mean(1) - t                     # noqa: E731
        p0 = np.log(t) / flat.mean(1).log()
        p1 = p0 * (1 + 1e-4) + 1e-4
        q0, q1 = f(p0), f(p1)
        for _ in range(12):
            p = torch.where(q1 != q0, p1 - q1 * (p1 - p0) / (q1 - q0), p1)
            p0, q0, p1 = p1, q1, p
            q1 = f(p1)
        return to_rgb((flat ** p1.clamp(0.1, 10)[:, None]).float().reshape(L.shape), a, b)

    return match, gamma


def accuracy(dev):
    import photometric_ref as R
    from oracle import clahe_oracle as C
    out = {}
    x = images(3, 2, 256, 256)
    x[0] *= 0.04
    ref, bound = R.lab_f64((x * 0.5 + 0.5).numpy().transpose(0, 2, 3, 1))
    light = photometric.lightness((x * 0.5 + 0.5).to(dev)).cpu().numpy()
    out["lightness_max_ratio_to_bound"] = {"shape": "2x3x256x256 (one image dark)", "ratio": float((np.abs(light - ref[..., 0]) / np.maximum(bound[..., 0], 1e-300)).max()),
                                           "max_abs_difference_to_float64": float(np.abs(light - ref[..., 0]).max()), "gate": 2.0}
    pure = {}
    for shape in ((3, 64, 64), (2, 100, 130)):
        x = images(7 + shape[1], *shape)
        xd = x.to(dev)
        for op, run, chan in (("match_histogram eq", lambda: photometric.match_histogram(xd, "eq", PAIR, PAIR), lambda c: P.channel_histogram_matching(c, "eq")),
                              ("match_histogram " + NAME, lambda: photometric.match_histogram(xd, NAME, PAIR, PAIR), lambda c: P.channel_histogram_matching(c, NAME)),
                              ("gamma_equalize 0.3", lambda: photometric.gamma_equalize(xd, 0.3, PAIR, PAIR), lambda c: P.channel_gamma_matching(c, 0.3))):
            got = run().cpu().numpy()
            ref = np.empty_like(got)
            for i in range(shape[0]):
                spc = C.rgb2normspace_lab((x[i].numpy() * 0.5 + 0.5).transpose(1, 2, 0).astype(np.float32))
                spc[:, :, 0] = chan(spc[:, :, 0])
                ref[i] = (C.normspace2rgb_lab(spc).transpose(2, 0, 1) - 0.5) / 0.5
            diff = np.abs(got - ref)
            pure["%s %dx3x%dx%d" % ((op,) + shape)] = {"max": float(diff.max()), "median": float(np.median(diff)), "share_above_5e-4": float((diff > 5e-4).mean())}
    out["difference_to_pure_oracle_pipeline"] = pure
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photometric_1gpu.json"))
    ap.add_argument("--quick", action="store_true", help="one small shape, for a rehearsal")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("photometric_bench needs a GPU: nothing here is measured on the CPU")
    dev = torch.device("cuda:0")
    photometric.load_histograms(os.path.join(ROOT, "tests", "golden", "photometric.npz"))
    t_match, t_gamma = torch_ops(dev, NAME)
    result = {"device": torch.cuda.get_device_name(0), "timing": "median (min - max) of 5 event-timed windows of `iters` calls each, one process", "shapes": {}}
    for n, h, w in ([(8, 64, 64)] if args.quick else [(128, 256, 256), (4, 1024, 1024)]):
        x = images(0, n, h, w).to(dev)
        px = n * h * w
        plane = photometric.lightness(x, PAIR)
        rows = {}
        rows["match_histogram eq"] = timed(lambda: photometric.match_histogram(x, "eq", PAIR, PAIR))
        rows["match_histogram " + NAME] = timed(lambda: photometric.match_histogram(x, NAME, PAIR, PAIR))
        rows["gamma_equalize 0.3"] = timed(lambda: photometric.gamma_equalize(x, 0.3, PAIR, PAIR))
        for key, nbytes in (("match_histogram eq", 36), ("match_histogram " + NAME, 36), ("gamma_equalize 0.3", 44)):
            rows[key]["algorithmic_bytes_per_pixel"] = nbytes
            rows[key]["algorithmic_TB_per_s"] = round(nbytes * px / rows[key]["ms_median"] / 1e9, 3)
        rows["clahe_lab clip 1.0 grid 8 (38 B / pixel)"] = timed(lambda: clahe.clahe_lab(x, 1.0, 8, PAIR, PAIR))
        rows["clahe_lab clip 1.0 grid 8 (38 B / pixel)"]["algorithmic_TB_per_s"] = round(38 * px / rows["clahe_lab clip 1.0 grid 8 (38 B / pixel)"]["ms_median"] / 1e9, 3)
        rows["torch ops: match eq"] = timed(lambda: t_match(x, False))
        rows["torch ops: match " + NAME] = timed(lambda: t_match(x, True))
        rows["torch ops: gamma 0.3 (12 fixed secant steps)"] = timed(lambda: t_gamma(x, 0.3))
        stages = {"lightness plane (pass 1 of gamma_equalize)": timed(lambda: photometric.lightness(x, PAIR)),
                  "histogram256 of the plane (memset + histogram pass, no colour conversion)": timed(lambda: photometric.histogram256(plane)),
                  "match_channel eq on the plane (memset + histogram + table + apply)": timed(lambda: photometric.match_channel(plane, "eq")),
                  "gamma_channel 0.3 on the plane (solve + apply)": timed(lambda: photometric.gamma_channel(plane, 0.3)),
                  "to_lab": timed(lambda: photometric.to_lab(x, PAIR))}
        _, gam, evals = photometric.gamma_equalize(x, 0.3, PAIR, PAIR, return_gamma=True, return_evaluations=True)
        evals = evals.cpu().numpy()
        result["shapes"]["%dx3x%dx%d" % (n, h, w)] = {
            "calls": rows, "stages": stages,
            "gamma_solve": {"function_evaluations_min": int(evals.min()), "function_evaluations_max": int(evals.max()),
                            "function_evaluations_mean": float(evals.mean()), "gamma_min": float(gam.min()), "gamma_max": float(gam.max()),
                            "workgroups": n, "note": "one workgroup per image: %d of the chip's CUs have work during the solve" % n}}
    result["accuracy"] = accuracy(dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
