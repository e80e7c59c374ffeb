"""dev tool: GeM-ResNet-18 / -34 (BasicBlock trunks, synthetic weights) and the fused BasicBlock kernel (gandtr_amd/csrc/conv3x3_basic.hip) on one device.
Everything is compared inside this process, alternating the variants, after a warm-up of every variant; every figure is the median of 5 with min .. max:
  (a) the whole forward of both nets at 32 x 3 x 1024^2 in f16 with GDT_CONV_BASIC unset (the library's default), =0 (layer by layer) and =1 (fused where the
      planner's threshold allows: layer1's identity blocks), a sample = FORWARDS forwards between two events; descriptors/s; the GeM-ResNet-101 forward in the same
      process.  The knob is read whenever a geometry is planned, i.e. at every forward: one net per trunk serves all settings.  THE DEFAULT FOLLOWS THIS: fused is
      the default only if its median is below the layer-by-layer median by more than the larger of the two min .. max ranges ("decision");
  (b) one identity block at 32 x 64 x 256^2 as one fused launch against the two layer-by-layer launches, from the executor's per-op event profile
      (gdt_net_set_profiling): algorithmic FLOP/s (2 convs x 2 N H W 64 64 9), bytes/s of x in + y out, and which bound applies at the device's peaks;
  (c) the f16x3 forward of both nets.
Event-timed single ops leave idle gaps and run at higher clocks than a sustained run: (b) ranks kernels; (a) is what decides.
Prints one JSON line and writes it to the path given (default profiles/resnet_basic_1gpu.json).
usage: tools/resnet_basic_bench.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                     # noqa: E402

from gandtr_amd import engine                                    # noqa: E402
from gandtr_amd.tools import synth                               # noqa: E402

REPS, FORWARDS = 5, 8
GEOMETRY = (32, 1024, 1024)
BLOCK = (32, 256, 256)
NETS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}
KNOB, FUSED = "GDT_CONV_BASIC", 936064
PEAK_FLOPS, PEAK_BYTES = 2.5e15, 8.0e12                          # MI355X: dense fp16 MFMA, HBM3E
dev = torch.device("cuda:0")


def set_knob(value):
    if value is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = value


def timed(fn, count=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / count


def med(v, digits=4):
    v = sorted(v)
    return {"ms": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits)}


def alternating(variants):
    """variants: {label: callable running one forward}; REPS samples of FORWARDS forwards each, the variants taking turns -- in an order rotated from round to
    round, so that no variant always runs behind the same one (a sample behind a heavier forward measured 3 % slower than the same plan behind a lighter one)"""
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    keys = list(variants)
    for r in range(REPS):
        for k in keys[r % len(keys):] + keys[:r % len(keys)]:
            t[k].append(timed(variants[k], FORWARDS))
    return {k: med(v, 3) for k, v in t.items()}


def whole_forwards():
    n, h, w = GEOMETRY
    x = synth.synth_input(60, (n, 3, h, w)).to(dev)
    out = {}
    r101 = engine.build_embedder(synth.resnet101_state(0), dev)
    for arch, blocks in NETS.items():
        net = engine.build_embedder(synth.resnet_basic_state(0, blocks=blocks), dev)

        def run(value, net=net):
            set_knob(value)
            net.forward(x)

        row = alternating({"unset": lambda: run(None), "0": lambda: run("0"), "1": lambda: run("1")})
        for k in row:
            row[k]["descriptors_per_s"] = round(n / row[k]["ms"] * 1e3, 1)
        fused_count = {}
        for value in (None, "0", "1"):
            set_knob(value)
            fused_count["unset" if value is None else value] = net.basic_blocks_fused(n, h, w)
        set_knob("1")
        a = net.forward(x)[net.out_slot].clone()
        set_knob("0")
        b = net.forward(x)[net.out_slot]
        row["fused_blocks_planned"] = fused_count
        row["max_abs_descriptor_difference_fused_vs_layered"] = float((a - b).abs().max())
        f, l = row["1"], row["0"]
        spread = max(f["max"] - f["min"], l["max"] - l["min"])
        row["decision"] = {"layered_minus_fused_ms": round(l["ms"] - f["ms"], 3), "larger_min_max_range_ms": round(spread, 3), "fused_wins": bool(l["ms"] - f["ms"] > spread)}
        row["gflop"] = round(net.flops(n, h, w) / 1e9, 1)
        out[arch] = row
        del net
        torch.cuda.empty_cache()
    set_knob(None)
    out["resnet101"] = alternating({"forward": lambda: r101.forward(x)})["forward"]
    out["resnet101"]["descriptors_per_s"] = round(n / out["resnet101"]["ms"] * 1e3, 1)
    return out


def one_block():
    n, h, w = BLOCK
    x = synth.synth_input(61, (n, 3, h, w)).to(dev)
    net = engine.HipNet(dev, "f16")
    t = net.conv(net.input(3), synth._normal(1, "w0", (64, 3, 1, 1), 0.5), synth._normal(1, "b0", (64,), 0.3), relu=True)
    sd = {}
    synth._bn(sd, 1, "bn1", 64)
    synth._bn(sd, 1, "bn2", 64, 0.25)
    bn = lambda p: tuple(sd[p + k] for k in (".weight", ".bias", ".running_mean", ".running_var"))
    hmid = net.conv(t, synth._normal(1, "w1", (64, 64, 3, 3), 576 ** -0.5), None, bn=bn("bn1"), pad=1, relu=True)
    y = net.conv(hmid, synth._normal(1, "w2", (64, 64, 3, 3), 576 ** -0.5), None, bn=bn("bn2"), pad=1, relu=True, residual=t)
    net.output_nchw(net.conv(y, synth._normal(1, "w3", (8, 64, 1, 1), 0.1)))
    net.finalize()
    net.set_profiling(True)
    times = {"fused": [], "layered": []}
    ran = {}
    for value in ("2", "0"):
        set_knob(value)
        for _ in range(2):
            net.forward(x)
    torch.cuda.synchronize()
    for _ in range(REPS):
        for label, value in (("fused", "2"), ("layered", "0")):
            set_knob(value)
            net.forward(x)
            torch.cuda.synchronize()
            convs = [(v, ms) for k, v, ms, fl in net.profile() if k == 1]
            ran[label] = [v for v, _ in convs]
            times[label].append(convs[1][1] + convs[2][1])           # the block's two conv ops (a skipped op times 0)
    set_knob(None)
    assert ran["fused"].count(FUSED) == 1 and FUSED not in ran["layered"], ran
    flop = 2 * 2.0 * n * h * w * 64 * 64 * 9
    nbytes = 2 * 2.0 * n * h * w * 64
    out = {"conv_variants": ran, "gflop": round(flop / 1e9, 1), "mbytes_x_in_y_out": round(nbytes / 1e6, 1),
           "least_ms_at_peak": {"flops": round(flop / PEAK_FLOPS * 1e3, 4), "bytes": round(nbytes / PEAK_BYTES * 1e3, 4),
                                "bound": "compute" if flop / PEAK_FLOPS > nbytes / PEAK_BYTES else "memory"}}
    for label in times:
        m = med(times[label])
        m["tflops"] = round(flop / m["ms"] / 1e9, 1)
        m["tb_per_s_x_in_y_out"] = round(nbytes / m["ms"] / 1e9, 3)
        out[label] = m
    out["layered_over_fused"] = round(out["layered"]["ms"] / out["fused"]["ms"], 3)
    return out


def exact_forwards():
    n, h, w = GEOMETRY
    x = synth.synth_input(60, (n, 3, h, w)).to(dev)
    out = {}
    for arch, blocks in NETS.items():
        net = engine.build_embedder(synth.resnet_basic_state(0, blocks=blocks), dev, precision="f16x3")
        for _ in range(2):
            net.forward(x)
        torch.cuda.synchronize()
        out[arch] = med([timed(lambda: net.forward(x), 4) for _ in range(REPS)], 3)
        out[arch]["descriptors_per_s"] = round(n / out[arch]["ms"] * 1e3, 1)
        del net
        torch.cuda.empty_cache()
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "resnet_basic_1gpu.json")
    out = {"workload": "GeM-ResNet-18 / -34, synthetic weights, forward at %d x 3 x %d x %d; medians of %d samples with min .. max, a whole-forward sample = %d forwards"
                       % (GEOMETRY + (REPS, FORWARDS)),
           "one_block_%dx64x%dx%d" % BLOCK: one_block(), "whole_forward_f16": whole_forwards(), "whole_forward_f16x3": exact_forwards()}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
