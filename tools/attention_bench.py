"""dev tool: the attention and edge-map embedders against the plain GeM embedder (the yardstick) on one device, default mode (f16), synthetic weights.
Per trunk, in one process: (1) the plain GeM forward, the attention forward (l2norm, normalize_max) and the one-channel + EdgeFilter forward, alternating
after a warm-up; (2) the two new kernels alone on a map of the trunk's output geometry (gdt_pixel_attention + gdt_pool_regions_weighted, GeM p = 3)
against the reference's op sequence for the same step in torch ops on the same device (pow / sum / sqrt / max / div / mul + clamp / pow / avg_pool2d /
pow), on the reference's own tensor (fp32 NCHW) and on the tensor the kernels read (fp16, channels-last memory), alternating.  Prints one JSON line.
usage: tools/attention_bench.py [iters] [arch ...]      (default 20 timed forwards per configuration; vgg16 and resnet101 at 32 x C x 1024 x 1024)"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch                                                     # noqa: E402
import torch.nn.functional as F                                  # noqa: E402

from gandtr_amd import engine                                    # noqa: E402
from gandtr_amd.tools import synth                               # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
archs = sys.argv[2:] or ["vgg16", "resnet101"]
dev = torch.device("cuda:0")
G = (32, 1024, 1024)
INNER = 20                                                       # calls per timed window of the kernel-level rows (one call is tens of microseconds)
FILTER = ("edgefilter", 10.0, 0.5, 500.0, 0.1, 1e-6)


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


def alternate(fns, n, reps=1):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(n):                                            # alternating: all see the same clocks / neighbours
        for k, fn in fns.items():
            t[k].append(timed(fn, reps))
    return {k: stats(v) for k, v in t.items()}


def torch_sequence(x, p=3.0, eps=1e-6):
    """CirRetrievalNetAttention.forward behind the trunk, batched: per-image L2-norm attention and maximum, feats * att, GeM"""
    m = (x.pow(2.0).sum(1) + 1e-10).sqrt()
    m = m / m.flatten(1).max(dim=1).values.view(-1, 1, 1)
    o = x * m.unsqueeze(1)
    return F.avg_pool2d(o.clamp(min=eps).pow(p), (o.size(-2), o.size(-1))).pow(1.0 / p)


out = {"workload": "attention / edge-map embedders vs plain GeM, f16, synthetic weights, %d x C x %d x %d" % G, "iters": iters, "archs": {}}
x3 = synth.synth_input(60, (G[0], 3, G[1], G[2])).to(dev)
x1 = synth._uniform(61, "edge.image", (G[0], 1, G[1], G[2]), 0.0, 1.0).to(dev)
for arch in archs:
    sd = synth.resnet101_state(0) if arch == "resnet101" else synth.vgg16_state(0)
    sd1 = dict(sd)
    sd1["features.0.weight"] = sd["features.0.weight"].sum(dim=1, keepdim=True)
    nets = {"gem": (engine.build_embedder(sd, dev), x3),
            "gem+attention": (engine.build_embedder(sd, dev, attention=("l2norm", True)), x3),
            "1 channel + edgefilter": (engine.build_embedder(sd1, dev, preprocessing=FILTER), x1)}
    row = alternate({k: (lambda net=net, x=x: net.forward(x)) for k, (net, x) in nets.items()}, iters)
    for k, (net, x) in nets.items():
        net.set_profiling(True)                                   # one profiled forward: the input pack and the first conv from the per-op events
        net.forward(x)
        torch.cuda.synchronize()
        p = net.profile()
        net.set_profiling(False)
        row[k]["input_pack_ms"] = round(sum(ms for kind, _, ms, _ in p if kind == 0), 3)
        row[k]["first_conv_ms"] = round([ms for kind, _, ms, _ in p if kind == 1][0], 3)
        row[k]["first_conv_variant"] = [v for kind, v, _, _ in p if kind == 1][0]
        row[k]["plan"] = {kk: v for kk, v in net.plan_summary(*G).items() if v}
        row[k]["head_launches"], row[k]["attention_launches"] = list(net.head_launches(*G)), list(net.attention_launches(*G))
        row[k]["over_plain_gem"] = round(row[k]["ms_median"] / row["gem"]["ms_median"], 4)
    del nets
    torch.cuda.empty_cache()

    # the step behind the trunk alone, on a map of the trunk's output geometry (post-ReLU values)
    d, s = (2048, 32) if arch == "resnet101" else (512, 16)
    h, w = G[1] // s, G[2] // s
    fmap = torch.relu(synth.synth_input(62, (G[0], d, h, w), name="map")).to(dev)             # fp32 NCHW: the reference's tensor
    nhwc16 = fmap.permute(0, 2, 3, 1).contiguous().half()                                     # what the f16 net's head reads
    nchw16_view = nhwc16.permute(0, 3, 1, 2)                                                  # the same memory under torch's NCHW indexing

    def pair():
        return engine.pool_regions_weighted(nhwc16, engine.pixel_attention(nhwc16, True), "gem", p=3.0)

    k = alternate({"kernel_pair": pair, "attention_kernel": lambda: engine.pixel_attention(nhwc16, True),
                   "torch_fp32_nchw": lambda: torch_sequence(fmap), "torch_fp16_channels_last": lambda: torch_sequence(nchw16_view)}, iters, INNER)
    ref = torch_sequence(fmap.half().float()).flatten(1)
    k["kernel_pair_max_abs_diff_to_torch"] = float((pair().flatten(1) - ref).abs().max())
    k["map"] = [G[0], h, w, d]
    fastest_torch = min(k["torch_fp32_nchw"]["ms_median"], k["torch_fp16_channels_last"]["ms_median"])
    k["kernel_pair_not_slower_than_torch"] = bool(k["kernel_pair"]["ms_median"] <= fastest_torch)
    row["head_step_alone"] = k
    extra = row["gem+attention"]["ms_median"] - row["gem"]["ms_median"]
    row["attention_forward_minus_plain_ms"] = round(extra, 4)
    row["attention_extra_within_torch_sequence"] = bool(extra <= fastest_torch)
    out["archs"][arch] = row
    del fmap, nhwc16, nchw16_view
    torch.cuda.empty_cache()
print(json.dumps(out))
