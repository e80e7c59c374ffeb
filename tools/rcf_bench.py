"""dev tool: RCF forward against HED (the two edge detectors of the ICCV23 scenarios) on one device, default mode (f16), synthetic weights.
Both nets run in the same process, alternating, after a warm-up of every geometry; then one profiled forward of each gives the per-op breakdown
(gdt_net_set_profiling: HIP events around every op).  Prints one JSON line.
usage: tools/rcf_bench.py [iters]      (default 20 timed forwards per net and geometry)"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch                                                     # noqa: E402

from gandtr_amd import engine                                    # noqa: E402
from gandtr_amd.tools import synth                               # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device("cuda:0")
GEOMETRIES = ((64, 256, 256), (8, 362, 481))
nets = {"rcf": engine.build_rcf(synth.rcf_state(0), dev), "hed": engine.build_hed(synth.hed_state(0), dev)}
inputs = {g: (synth.synth_input(50, (g[0], 3, g[1], g[2]), 1.0) * 127.5).to(dev) for g in GEOMETRIES}
for g in GEOMETRIES:
    for net in nets.values():
        for _ in range(3):
            net.forward(inputs[g])
torch.cuda.synchronize()

# RCF op order (engine.build_rcf): input, conv1_1, conv1_2, pool1, conv2_1, conv2_2, pool2, conv3_1-3, pool3, conv4_1-3, pool4 (stride 1), conv5_1-3, head
RCF_GROUPS = {"input": [0], "conv1": [1, 2], "conv2": [4, 5], "conv3": [7, 8, 9], "conv4": [11, 12, 13], "conv5_dilated": [15, 16, 17],
              "pools": [3, 6, 10, 14], "head": [18]}


def timed(net, x):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    net.forward(x)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


out = {"workload": "RCF vs HED forward, f16, synthetic weights, Caffe-range input", "iters": iters, "geometries": {}}
for g in GEOMETRIES:
    n = g[0]
    t = {k: [] for k in nets}
    for _ in range(iters):                                          # alternating: both see the same clocks / neighbours
        for k, net in nets.items():
            t[k].append(timed(net, inputs[g]))
    row = {}
    for k, net in nets.items():
        v = sorted(t[k])
        med = v[len(v) // 2]
        gf = net.flops(*g) / 1e9
        row[k] = {"ms_median": round(med, 3), "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3), "images_per_s": round(n / med * 1e3, 1),
                  "gflop_per_image": round(gf / n, 2), "tflops": round(gf / med, 1)}
    row["rcf_over_hed"] = round(row["rcf"]["ms_median"] / row["hed"]["ms_median"], 3)
    prof = {}
    for k, net in nets.items():
        net.set_profiling(True)
        net.forward(inputs[g])
        torch.cuda.synchronize()
        p = net.profile()
        net.set_profiling(False)
        total = sum(ms for _, _, ms, _ in p)
        if k == "rcf":
            br = {name: round(sum(p[i][2] for i in idx), 3) for name, idx in RCF_GROUPS.items()}
            br["variants_conv5"] = [p[i][1] for i in RCF_GROUPS["conv5_dilated"]]
            br["head_share"] = round(br["head"] / total, 4)
        else:
            br = {"convs": round(sum(ms for kind, _, ms, _ in p if kind == 1), 3), "pools": round(sum(ms for kind, _, ms, _ in p if kind == 3), 3),
                  "head": round(sum(ms for kind, _, ms, _ in p if kind == 6), 3)}
        br["sum_of_ops_ms"] = round(total, 3)
        prof[k] = br
    row["profile_ms"] = prof
    row["workspace_gb"] = {k: round(net.workspace_bytes(*g) / 1e9, 3) for k, net in nets.items()}
    out["geometries"]["%dx3x%dx%d" % g] = row
print(json.dumps(out))
