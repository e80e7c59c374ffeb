"""dev tool: the PatchGAN discriminator (NLayerDiscriminator, ndf 64, 3 layers) behind the generator on one device: 64 x 3 x 256^2, f16, synthetic weights,
InstanceNorm and BatchNorm nets.  Everything is compared inside this process, alternating, after a warm-up of every variant:
  * the whole forward with the 4x4 patch kernel (conv4x4_halo.hip) and with GDT_CONV4X4_HALO=0 (the generic implicit-GEMM path), event-timed;
  * the per-layer times of both from the executor's per-op event profile (gdt_net_set_profiling), five profiled forwards each, averaged;
  * generator (default mode, f16c) followed by the discriminator on its output against the generator alone.
Event-timed single forwards leave idle gaps and run at higher clocks than a sustained run: they rank kernels; bench.py quotes speed.
Prints one JSON line and writes it to the path given (default profiles/discriminator_bench_1gpu.json).
usage: tools/discriminator_bench.py [iters] [out.json]      (default 20 timed forwards per variant)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                     # noqa: E402

from gandtr_amd import engine                                    # noqa: E402
from gandtr_amd.tools import synth                               # noqa: E402

KNOB = "GDT_CONV4X4_HALO"
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "discriminator_bench_1gpu.json")
dev = torch.device("cuda:0")
G = (64, 256, 256)
nets = {norm: engine.build_discriminator(synth.discriminator_state(0, norm, gain=0.2 if norm == "instance" else None), dev) for norm in ("instance", "batch")}
gen = engine.build_generator(synth.generator_state(0, "instance"), dev)
x = synth.synth_input(50, (G[0], 3, G[1], G[2]), 1.0).to(dev)


def knob(on):
    if on:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = "0"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    v = sorted(v)
    return {"ms_median": round(v[len(v) // 2], 3), "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3)}


def conv_rows(net):
    """per conv op of five profiled forwards, averaged: (variant, ms, flops)"""
    runs = []
    for _ in range(5):
        net.set_profiling(True)
        net.forward(x)
        torch.cuda.synchronize()
        runs.append(net.profile())
        net.set_profiling(False)
    rows = []
    for i, (kind, variant, _, fl) in enumerate(runs[0]):
        ms = sum(r[i][2] for r in runs) / len(runs)
        rows.append((kind, variant, ms, fl))
    return rows


for on in (True, False):                                            # warm-up of every variant
    knob(on)
    for net in nets.values():
        for _ in range(3):
            net.forward(x)
knob(True)
for _ in range(3):
    fake = gen.forward(x)[gen.out_slot]
torch.cuda.synchronize()

out = {"workload": "NLayerDiscriminator(ndf 64, 3 layers) forward, f16, 64x3x256x256, synthetic weights; generator f16c", "iters": iters,
       "gflop_per_image": round(nets["instance"].flops(*G) / G[0] / 1e9, 3), "nets": {}}
for norm, net in nets.items():
    t = {True: [], False: []}
    for _ in range(iters):
        for on in (True, False):
            knob(on)
            t[on].append(timed(lambda: net.forward(x)))
    row = {"patch_kernel": stats(t[True]), "generic": stats(t[False])}
    gf = net.flops(*G) / 1e9
    for k in ("patch_kernel", "generic"):
        row[k]["tflops"] = round(gf / row[k]["ms_median"], 1)
    row["generic_over_patch"] = round(row["generic"]["ms_median"] / row["patch_kernel"]["ms_median"], 3)
    prof = {}
    for on in (True, False):
        knob(on)
        prof[on] = conv_rows(net)
    layers, li = {}, 0
    for (kind, var_on, ms_on, fl), (_, var_off, ms_off, _) in zip(prof[True], prof[False]):
        if kind != 1:
            continue
        li += 1
        layers["layer%d" % li] = {"gflop": round(fl / 1e9, 2), "patch_variant": var_on, "patch_ms": round(ms_on, 4), "patch_tflops": round(fl / 1e9 / ms_on, 1) if ms_on > 0 else 0,
                                  "generic_variant": var_off, "generic_ms": round(ms_off, 4), "generic_tflops": round(fl / 1e9 / ms_off, 1) if ms_off > 0 else 0,
                                  "generic_over_patch": round(ms_off / ms_on, 3) if ms_on > 0 else 0}
    row["layers"] = layers
    row["other_ops_ms"] = {"patch_kernel": round(sum(r[2] for r in prof[True] if r[0] != 1), 4), "generic": round(sum(r[2] for r in prof[False] if r[0] != 1), 4)}
    knob(True)
    row["conv4x4_launches"] = net.conv4x4_launches(*G)
    row["workspace_gb"] = round(net.workspace_bytes(*G) / 1e9, 3)
    out["nets"][norm] = row
knob(True)

# generator alone against generator + discriminator on its output (same stream, no host copy in between)
disc = nets["instance"]
tg, tgd = [], []
for _ in range(iters):
    tg.append(timed(lambda: gen.forward(x)))
    tgd.append(timed(lambda: disc.forward(gen.forward(x)[gen.out_slot])))
sg, sgd = stats(tg), stats(tgd)
out["generator_then_discriminator"] = {"generator": sg, "generator_discriminator": sgd,
                                       "overhead_ms": round(sgd["ms_median"] - sg["ms_median"], 3), "overhead_share": round(sgd["ms_median"] / sg["ms_median"] - 1, 4)}
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
