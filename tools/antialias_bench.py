"""dev tool: the anti-aliased ResnetGenerator (CUT's defaults, synthetic weights) and its blur-resample kernels (gandtr_amd/csrc/blur_resample.hip) on one device.
Everything but the knob comparison is compared inside this process, alternating, after a warm-up of every variant; every figure is the median of 5 with min .. max:
  * both kernels alone at the generator's own shapes at batch 64 -- down 256^2 x 128 and 128^2 x 256 channels, up 64^2 x 256 and 128^2 x 128 channels -- with fp16
    and fp32 tensors, plain and norm-folded, from the executor's per-op event profile (gdt_net_set_profiling); TB/s of algorithmic bytes (input once + output once);
    comparators: the same function in torch ops on the same GPU (channels-last; F.pad + depthwise F.conv2d, F.interpolate) and, for the up kernel, gdt_k_resize on the
    same shape in the same forward;
  * folded against unfolded: GDT_NORM_FUSION is latched, so one child process per setting runs the whole forward (f16c, f16x3) and its per-op profile; reported are the
    three InstanceNorm ops in front of a blur op and the blur ops in both settings (unfolded norm - folded norm = the apply pass that went away) and the whole forwards
    (the knob also unfolds the convs' norms: that difference is not the blur fold's alone);
  * the whole forward at 64 x 3 x 256^2 in f16c, f16 and f16x3 against the hub-configuration generator, with the FLOPs of both (the stride-1 convs do four times the
    work of the stride-2 ones) and the kernel variant of every conv.
Event-timed single forwards leave idle gaps and run at higher clocks than a sustained run: they rank kernels; bench.py quotes speed.
Prints one JSON line and writes it to the path given (default profiles/antialias_1gpu.json).
usage: tools/antialias_bench.py [out.json]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                     # noqa: E402
import torch.nn.functional as F                                  # noqa: E402

from gandtr_amd import engine                                    # noqa: E402
from gandtr_amd.tools import synth                               # noqa: E402

REPS = 5
GEOMETRY = (64, 256, 256)
KIND_NORM, KIND_RESIZE, KIND_BLUR = 2, 11, 12
dev = torch.device("cuda:0")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def med(v, digits=4):
    v = sorted(v)
    return {"ms": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits)}


def profiled(net, x):
    net.set_profiling(True)
    net.forward(x)
    torch.cuda.synchronize()
    rows = net.profile()
    net.set_profiling(False)
    return rows


def aa_state(**kw):
    return synth.generator_state(0, "instance", no_antialias=False, no_antialias_up=False, **kw)


def child():
    """one knob setting (the environment's): whole forwards and per-op profiles of the anti-aliased generator, as one JSON line"""
    n, h, w = GEOMETRY
    x = synth.synth_input(50, (n, 3, h, w), 1.0).to(dev)
    res = {}
    for prec in ("f16c", "f16x3"):
        net = engine.build_generator(aa_state(), dev, precision=prec)
        for _ in range(2):
            net.forward(x)
        torch.cuda.synchronize()
        t = [timed(lambda: net.forward(x)) for _ in range(REPS)]
        runs = [profiled(net, x) for _ in range(REPS)]
        kinds = [r[0] for r in runs[0]]
        blur = [j for j, k in enumerate(kinds) if k == KIND_BLUR]
        norms = [max(i for i in range(j) if kinds[i] == KIND_NORM) for j in blur[:2] + blur[3:]]      # the norms in front of both Downsamples and of the second Upsample
        res[prec] = {"forward": med(t, 3), "blur_summary": net.blur_summary(*GEOMETRY), "norms_folded": net.plan_summary(*GEOMETRY)["norms_folded"],
                     "blur_ops_ms": [med([run[j][2] for run in runs]) for j in blur], "norm_ops_in_front_ms": [med([run[j][2] for run in runs]) for j in norms],
                     "profile_total_ms": med([sum(r[2] for r in run) for run in runs], 3)}
        del net
        torch.cuda.empty_cache()
    print("CHILD " + json.dumps(res))


def kernels_alone():
    """the ops at the generator's shapes: 1 x 1 conv (3 -> C) -> [InstanceNorm + ReLU] -> op -> 1 x 1 conv (C -> 8) -> tap"""
    out = {}
    n = GEOMETRY[0]
    for up, c, s in ((False, 128, 256), (False, 256, 128), (True, 256, 64), (True, 128, 128)):
        x = synth.synth_input(50, (n, 3, s, s), 1.0).to(dev)
        so = 2 * s if up else s // 2
        for prec, dtype, es in (("f16", torch.float16, 2), ("f16x3", torch.float32, 4)):
            nbytes = float(es) * n * c * (s * s + so * so)
            entry = {"mbytes": round(nbytes / 1e6, 1)}
            for form in ("plain", "folded"):
                net = engine.HipNet(dev, prec)
                raw = net.conv(net.input(3), synth._normal(1, "wa", (c, 3, 1, 1), 0.7), None if form == "folded" else synth._normal(1, "ba", (c,), 0.5))
                t = net.instance_norm(raw, relu=True) if form == "folded" else raw
                y = net.blur_resample(t, up=up)
                net.output_nchw(net.conv(y, synth._normal(1, "wc", (8, c, 1, 1), 0.1)))
                if up and form == "plain":            # gdt_k_resize on the same tensor to the same size, in the same forward
                    net.output_nchw(net.conv(net.resize(raw, y, "bilinear"), synth._normal(1, "wd", (8, c, 1, 1), 0.1)))
                net.finalize()
                assert net.blur_summary(n, s, s)["folded"] == (1 if form == "folded" else 0)
                for _ in range(2):
                    net.forward(x)
                runs = [profiled(net, x) for _ in range(REPS)]
                kinds = [r[0] for r in runs[0]]
                j = kinds.index(KIND_BLUR)
                entry[form] = med([run[j][2] for run in runs])
                entry[form]["tb_per_s"] = round(nbytes / entry[form]["ms"] / 1e9, 2)
                if form == "folded":
                    entry["folded_norm_statistics_op"] = med([run[kinds.index(KIND_NORM)][2] for run in runs])
                elif up:
                    jr = kinds.index(KIND_RESIZE)
                    entry["gdt_k_resize"] = med([run[jr][2] for run in runs])
                    entry["gdt_k_resize"]["tb_per_s"] = round(nbytes / entry["gdt_k_resize"]["ms"] / 1e9, 2)
                    entry["resize_over_kernel"] = round(entry["gdt_k_resize"]["ms"] / entry["plain"]["ms"], 3)
                del net
                torch.cuda.empty_cache()
            xt = torch.randn(n, c, s, s, device=dev, dtype=dtype).contiguous(memory_format=torch.channels_last)
            if up:
                fn = lambda: F.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=False)
            else:
                filt = (torch.tensor([1., 2., 1.])[:, None] * torch.tensor([1., 2., 1.])[None, :] / 16).to(dev, dtype)[None, None].repeat(c, 1, 1, 1)
                fn = lambda: F.conv2d(F.pad(xt, (1, 1, 1, 1), mode="reflect"), filt, stride=2, groups=c)
            for _ in range(2):
                fn()
            entry["torch"] = med([timed(fn) for _ in range(REPS)])
            entry["torch"]["tb_per_s"] = round(nbytes / entry["torch"]["ms"] / 1e9, 2)
            entry["torch_over_kernel"] = round(entry["torch"]["ms"] / entry["plain"]["ms"], 3)
            out["%s %dx%dx%dx%d %s" % ("up" if up else "down", n, c, s, s, prec)] = entry
            del xt
            torch.cuda.empty_cache()
    return out


def whole_forwards():
    n, h, w = GEOMETRY
    x = synth.synth_input(50, (n, 3, h, w), 1.0).to(dev)
    out = {}
    for prec in ("f16c", "f16", "f16x3"):
        nets = {"antialiased": engine.build_generator(aa_state(), dev, precision=prec), "hub": engine.build_generator(synth.generator_state(0, "instance"), dev, precision=prec)}
        for net in nets.values():
            for _ in range(2):
                net.forward(x)
        torch.cuda.synchronize()
        t = {k: [] for k in nets}
        for _ in range(REPS):
            for k, net in nets.items():
                t[k].append(timed(lambda: net.forward(x)))
        row = {}
        for k, net in nets.items():
            prof = profiled(net, x)
            row[k] = {"forward": med(t[k], 3), "gflop": round(net.flops(*GEOMETRY) / 1e9, 1), "workspace_gb": round(net.workspace_bytes(*GEOMETRY) / 1e9, 3),
                      "plan": {p: v for p, v in net.plan_summary(*GEOMETRY).items() if v}, "blur_summary": net.blur_summary(*GEOMETRY),
                      "conv_variants_ms_gflop": [[r[1], round(r[2], 3), round(r[3] / 1e9, 1)] for r in prof if r[0] == 1],
                      "blur_ops_ms": [round(r[2], 3) for r in prof if r[0] == KIND_BLUR]}
            row[k]["tflops"] = round(row[k]["gflop"] / row[k]["forward"]["ms"], 1)
        row["antialiased_over_hub_ms"] = round(row["antialiased"]["forward"]["ms"] / row["hub"]["forward"]["ms"], 3)
        row["antialiased_over_hub_flop"] = round(row["antialiased"]["gflop"] / row["hub"]["gflop"], 3)
        out[prec] = row
        del nets
        torch.cuda.empty_cache()
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "antialias_1gpu.json")
    out = {"workload": "ResnetGenerator(no_antialias=False, no_antialias_up=False), 9 blocks, InstanceNorm, synthetic weights, forward at %d x 3 x %d x %d; medians of %d "
                       "with min .. max" % (GEOMETRY + (REPS,))}
    fusion = {}
    for label, value in (("folded", None), ("GDT_NORM_FUSION=0", "0")):
        env = {k: v for k, v in os.environ.items() if k != "GDT_NORM_FUSION"}
        if value is not None:
            env["GDT_NORM_FUSION"] = value
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True, capture_output=True, text=True)
        fusion[label] = json.loads(next(l for l in p.stdout.splitlines() if l.startswith("CHILD "))[6:])
    for prec in fusion["folded"]:
        a, b = fusion["folded"][prec], fusion["GDT_NORM_FUSION=0"][prec]
        apply_ms = sum(u["ms"] - f["ms"] for u, f in zip(b["norm_ops_in_front_ms"], a["norm_ops_in_front_ms"]))
        blur_ms = sum(f["ms"] for f in a["blur_ops_ms"]) - sum(u["ms"] for u in b["blur_ops_ms"])
        fusion["summary " + prec] = {"apply_passes_removed_ms": round(apply_ms, 4), "blur_ops_slower_by_ms": round(blur_ms, 4), "net_gain_of_the_blur_folds_ms": round(apply_ms - blur_ms, 4),
                                     "whole_forward_gain_ms_all_folds": round(b["forward"]["ms"] - a["forward"]["ms"], 3)}
    out["folded_against_unfolded"] = fusion
    out["kernels_alone"] = kernels_alone()
    out["whole_forward"] = whole_forwards()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    child() if "--child" in sys.argv[1:] else main()
