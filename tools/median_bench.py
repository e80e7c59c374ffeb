"""dev tool: the geometric-median (Weiszfeld) pooling on one device, synthetic data.  In one process, every figure a median of 5 timed windows with min-max:
(1) gdt_geometric_median alone on fp16 NHWC maps of the trunks' output geometries (32 x 32 x 32 x 2048, 32 x 64 x 64 x 512) for 0, 3 and 10 iterations, with
    its bytes/s against the (T + 1) map reads the algorithm needs (the partial sums it writes and reads back are not counted);
(2) the reference's op sequence for the same step in torch ops on the same device, on the reference's own tensor (fp32 NCHW): as the reference runs it
    (image by image: it cannot take a batch) and as a batched restatement; alternating with (1);
(3) the whole forward of GeM-VGG16 and GeM-ResNet-101 at 32 x 3 x 1024 x 1024 (f16, synthetic weights) with the median head (3 iterations) against the
    plain GeM forward, alternating.
Writes the JSON to the path given (default profiles/median_pool_1gpu.json) and prints it.
usage: tools/median_bench.py [out.json] [windows]"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch                                                     # noqa: E402

from gandtr_amd import engine                                    # noqa: E402
from gandtr_amd.components.model.layers import pooling           # noqa: E402
from gandtr_amd.tools import synth                               # noqa: E402

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "median_pool_1gpu.json")
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 5
assert torch.cuda.is_available(), "median_bench needs a GPU"
dev = torch.device("cuda:0")
MAPS = ((32, 32, 32, 2048), (32, 64, 64, 512))                    # N, H, W, D
ITERATIONS = (0, 3, 10)
G = (32, 1024, 1024)
HEAD_ITERATIONS = 3
INNER = 10                                                       # kernel calls per timed window


def timed(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(v):
    v = sorted(v)
    return {"ms_median": round(v[len(v) // 2], 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4)}


def alternate(fns, n):
    """fns: {name: (callable, calls per window)}; a warm-up of every callable, then n windows each, alternating: all see the same clocks / neighbours"""
    for fn, _ in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(n):
        for k, (fn, reps) in fns.items():
            t[k].append(timed(fn, reps))
    return {k: stats(v) for k, v in t.items()}


def torch_per_image(x, iterations):
    """as the reference runs it: one image at a time (layers/pooling.py, the reference's fp32 op sequence)"""
    return torch.cat([pooling.weiszfeld(x[i:i + 1], iterations) for i in range(x.size(0))])


def torch_batched(x, iterations):
    """the same iteration restated for a batch: per-image sums"""
    w = torch.ones((x.size(0), 1) + tuple(x.shape[2:]), device=x.device)
    for _ in range(iterations):
        m = (x * w).sum((2, 3), keepdim=True) / w.sum((2, 3), keepdim=True)
        w = 1.0 / ((x - m).pow(2.0).sum(1, keepdim=True) + 1e-10).sqrt()
    return (x * w).sum((2, 3), keepdim=True) / w.sum((2, 3), keepdim=True)


out = {"workload": "geometric-median pooling: kernel alone vs torch ops, and the median head inside the embedders, f16, synthetic data",
       "windows": windows, "kernel_calls_per_window": INNER, "maps": {}, "archs": {}}

for n, h, w, d in MAPS:
    fmap = torch.relu(synth.synth_input(70, (n, d, h, w), name="map")).to(dev)                # fp32 NCHW: the reference's tensor
    nhwc16 = fmap.permute(0, 2, 3, 1).contiguous().half()                                     # what the f16 net's head reads
    map_bytes = nhwc16.numel() * 2
    row = {"map_bytes_fp16": map_bytes}
    with torch.no_grad():
        for it in ITERATIONS:
            r = alternate({"kernel_fp16_nhwc": (lambda it=it: engine.geometric_median(nhwc16, it), INNER),
                           "torch_fp32_nchw_per_image": (lambda it=it: torch_per_image(fmap, it), 1),
                           "torch_fp32_nchw_batched": (lambda it=it: torch_batched(fmap, it), 1)}, windows)
            k = r["kernel_fp16_nhwc"]
            k["map_reads"] = it + 1
            for q in ("median", "min", "max"):                    # (the fastest window gives the highest rate)
                k["tb_per_s_" + q] = round((it + 1) * map_bytes / (k["ms_" + q] * 1e-3) / 1e12, 3)
            ref = torch_batched(fmap.half().float(), it).flatten(1)
            got = engine.geometric_median(nhwc16, it)
            r["kernel_max_abs_diff_to_torch"] = float((got - ref).abs().max())
            r["kernel_over_torch_per_image"] = round(k["ms_median"] / r["torch_fp32_nchw_per_image"]["ms_median"], 4)
            r["kernel_over_torch_batched"] = round(k["ms_median"] / r["torch_fp32_nchw_batched"]["ms_median"], 4)
            row["iterations_%d" % it] = r
    out["maps"]["%dx%dx%dx%d" % (n, h, w, d)] = row
    del fmap, nhwc16
    torch.cuda.empty_cache()

x3 = synth.synth_input(60, (G[0], 3, G[1], G[2])).to(dev)
for arch in ("vgg16", "resnet101"):
    sd = synth.resnet101_state(0) if arch == "resnet101" else synth.vgg16_state(0)
    nets = {"gem": engine.build_embedder(sd, dev), "median_%d" % HEAD_ITERATIONS: engine.build_embedder(sd, dev, head=("geometric_median", HEAD_ITERATIONS, False, False))}
    row = alternate({k: ((lambda net=net: net.forward(x3)), 1) for k, net in nets.items()}, windows)
    for k, net in nets.items():
        row[k]["head_launches"] = list(net.head_launches(*G))
        row[k]["over_plain_gem"] = round(row[k]["ms_median"] / row["gem"]["ms_median"], 4)
    out["archs"][arch] = row
    del nets
    torch.cuda.empty_cache()

text = json.dumps(out, indent=1)
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
with open(path, "w") as f:
    f.write(text + "\n")
print(json.dumps(out))
