"""dev tool: the pix2pix U-Net generator (UnetGenerator, num_downs 8, ngf 64) on one device: 64 x 3 x 256^2, synthetic weights, BatchNorm and InstanceNorm nets.
Everything is compared inside this process, alternating, after a warm-up of every variant:
  * the whole forward in f16 with the transposed 4x4 patch kernel (conv4x4t_halo.hip), with GDT_CONV4X4T_HALO=0 (copy of the concatenation + four phase launches
    of the generic implicit GEMM), and in f16x3 -- event-timed;
  * per up-convolution, from the executor's per-op event profile (gdt_net_set_profiling; five profiled forwards per variant, alternating, averaged): time of the patch
    kernel and of the generic route (its concatenation copy + its phase launches), algorithmic TFLOP/s, algorithmic bytes (both inputs, the
    output, the fp16 weights, each once) and the larger of the FLOP floor (2.5 PFLOP/s) and the HBM floor (8 TB/s) with the bound it names;
  * the ResNet generator's f16 forward on the same input, for scale.
Event-timed single forwards leave idle gaps and run at higher clocks than a sustained run: they rank kernels; bench.py quotes speed.
Prints one JSON line and writes it to the path given (default profiles/unet_bench_1gpu.json).
usage: tools/unet_bench.py [iters] [out.json]      (default 20 timed forwards per variant)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                     # noqa: E402

from gandtr_amd import engine                                    # noqa: E402
from gandtr_amd.tools import synth                               # noqa: E402

KNOB = "GDT_CONV4X4T_HALO"
PEAK_FLOPS, PEAK_BYTES = 2.5e15, 8.0e12
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "unet_bench_1gpu.json")
dev = torch.device("cuda:0")
G = (64, 256, 256)
NUM_DOWNS, NGF = 8, 64
VARIANTS = {"patch_kernel": None, "generic": "0"}
states = {norm: synth.unet_state(0, norm, ngf=NGF, num_downs=NUM_DOWNS) for norm in ("batch", "instance")}
nets = {(norm, prec): engine.build_unet_generator(states[norm], dev, precision=prec) for norm in states for prec in ("f16", "f16x3")}
resnet = engine.build_generator(synth.generator_state(0, "instance"), dev, precision="f16")
x = synth.synth_input(50, (G[0], 3, G[1], G[2]), 1.0).to(dev)


def knob(value):
    if value is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = value


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


def profiled(net):
    net.set_profiling(True)
    net.forward(x)
    torch.cuda.synchronize()
    rows = net.profile()
    net.set_profiling(False)
    return rows


def up_conv_shapes():
    """(cin_a, cin_b, cout, input h, input w) of the up-convolutions in graph order (innermost first)"""
    widths = [NGF * min(2 ** i, 8) for i in range(NUM_DOWNS)]
    rows = []
    for i in range(NUM_DOWNS - 1, -1, -1):
        side = G[1] >> (i + 1)
        rows.append((widths[i], 0 if i == NUM_DOWNS - 1 else widths[i], 3 if i == 0 else widths[i - 1], side, side))
    return rows


for value in VARIANTS.values():                                     # warm-up of every variant
    knob(value)
    for net in nets.values():
        for _ in range(3):
            net.forward(x)
knob(None)
for _ in range(3):
    resnet.forward(x)
torch.cuda.synchronize()

out = {"workload": "UnetGenerator(num_downs 8, ngf 64) forward, 64x3x256x256, synthetic weights", "iters": iters,
       "gflop_per_image": round(nets[("batch", "f16")].flops(*G) / G[0] / 1e9, 3), "nets": {}}
for norm in states:
    net, exact = nets[(norm, "f16")], nets[(norm, "f16x3")]
    t = {k: [] for k in VARIANTS}
    tx = []
    for _ in range(iters):
        for k, value in VARIANTS.items():
            knob(value)
            t[k].append(timed(lambda: net.forward(x)))
        knob(None)
        tx.append(timed(lambda: exact.forward(x)))
    gf = net.flops(*G) / 1e9
    row = {k: stats(v) for k, v in t.items()}
    row["f16x3"] = stats(tx)
    for k in row:
        row[k]["tflops"] = round(gf / row[k]["ms_median"], 1)
        row[k]["images_per_s"] = round(G[0] / row[k]["ms_median"] * 1e3, 1)
    row["generic_over_patch"] = round(row["generic"]["ms_median"] / row["patch_kernel"]["ms_median"], 3)
    # per up-convolution: five profiled forwards per variant, alternating
    prof = {k: [] for k in VARIANTS}
    for _ in range(5):
        for k, value in VARIANTS.items():
            knob(value)
            prof[k].append(profiled(net))
    knob(None)
    kinds = [r[0] for r in prof["generic"][0]]
    mean = lambda k, i: sum(run[i][2] for run in prof[k]) / len(prof[k])
    spread = lambda k, i: max(run[i][2] for run in prof[k]) - min(run[i][2] for run in prof[k])
    ups = [i for i, r in enumerate(prof["generic"][0]) if r[0] == 1 and r[3] > 0 and i > 0 and (kinds[i - 1] == 9 or any(907000 <= run[i][1] < 908000 for run in prof["patch_kernel"]))]
    shapes = up_conv_shapes()
    layers = {}
    for n_up, i in enumerate(ups):
        ca, cb, cout, h, w = shapes[n_up]
        fl = prof["generic"][0][i][3]
        by = 2.0 * G[0] * h * w * (ca + cb) + G[0] * 4.0 * h * w * cout * (4 if n_up == len(ups) - 1 else 2) + 2.0 * (ca + cb) * cout * 16      # (the outermost writes fp32)
        cat = i - 1 if kinds[i - 1] == 9 else None
        generic_ms = mean("generic", i) + (mean("generic", cat) if cat is not None else 0.0)
        floor_f, floor_b = fl / PEAK_FLOPS * 1e3, by / PEAK_BYTES * 1e3
        entry = {"cin_a": ca, "cin_b": cb, "cout": cout, "in_hw": [h, w], "gflop": round(fl / 1e9, 2), "mbytes": round(by / 1e6, 1),
                 "floor_ms": round(max(floor_f, floor_b), 4), "bound": "flop" if floor_f >= floor_b else "hbm",
                 "generic_ms": round(generic_ms, 4), "generic_concat_ms": round(mean("generic", cat), 4) if cat is not None else 0.0,
                 "generic_variant": prof["generic"][0][i][1], "generic_spread_ms": round(spread("generic", i), 4)}
        for k in ("patch_kernel",):
            ms = mean(k, i) + (mean(k, cat) if cat is not None else 0.0)
            entry[k] = {"variant": prof[k][0][i][1], "ms": round(ms, 4), "spread_ms": round(spread(k, i), 4), "tflops": round(fl / 1e9 / ms, 1) if ms > 0 else 0,
                        "floor_share": round(max(floor_f, floor_b) / ms, 3) if ms > 0 else 0, "generic_over_this": round(generic_ms / ms, 3) if ms > 0 else 0}
        entry["generic_tflops"] = round(fl / 1e9 / generic_ms, 1) if generic_ms > 0 else 0
        layers["up%d" % n_up] = entry
    row["up_convs"] = layers
    row["other_ops_ms"] = {k: round(sum(mean(k, i) for i in range(len(kinds)) if i not in ups and not (i + 1 in ups and kinds[i] == 9)), 4) for k in ("patch_kernel", "generic")}
    row["conv4x4t_launches"] = net.conv4x4t_launches(*G)
    row["conv4x4_launches"] = net.conv4x4_launches(*G)
    row["workspace_gb"] = {"f16": round(net.workspace_bytes(*G) / 1e9, 3), "f16x3": round(exact.workspace_bytes(*G) / 1e9, 3)}
    out["nets"][norm] = row

tr = [timed(lambda: resnet.forward(x)) for _ in range(iters)]
out["resnet_generator_f16"] = dict(stats(tr), gflop_per_image=round(resnet.flops(*G) / G[0] / 1e9, 3))
out["resnet_generator_f16"]["images_per_s"] = round(G[0] / out["resnet_generator_f16"]["ms_median"] * 1e3, 1)
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
