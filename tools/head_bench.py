"""dev tool: the descriptor heads against the plain GeM embedder (the yardstick) on one device, default mode (f16), synthetic weights.
The four configurations of a trunk run in the same process, alternating, after a warm-up; then one profiled forward of each gives the head's
ops from the executor's per-op events (gdt_net_set_profiling).  Prints one JSON line.
usage: tools/head_bench.py [iters] [arch ...]      (default 20 timed forwards per configuration; resnet101 and vgg16 at 32 x 3 x 1024 x 1024)"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch                                                     # noqa: E402

from gandtr_amd import engine                                    # noqa: E402
from gandtr_amd.tools import synth                               # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
archs = sys.argv[2:] or ["resnet101", "vgg16"]
dev = torch.device("cuda:0")
G = (32, 1024, 1024)
# (name, head tuple of ImageRetrievalNet._hip_head: pooling, regional, L, eps, local whitening, final whitening)
CONFIGS = (("gem", None), ("gem+whitening", ("gem", False, 0, 1e-6, False, True)), ("gem+regional+whitening", ("gem", True, 3, 1e-6, False, True)),
           ("gem+local_whitening", ("gem", False, 0, 1e-6, True, False)))
OP_CONV, OP_GEM, OP_POOL_HEAD = 1, 4, 8                          # op kinds of gdt_net_profile_read


def timed(net, x):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    net.forward(x)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


out = {"workload": "descriptor heads vs plain GeM, f16, synthetic weights, %d x 3 x %d x %d" % G, "iters": iters, "archs": {}}
x = synth.synth_input(60, (G[0], 3, G[1], G[2])).to(dev)
for arch in archs:
    sd = synth.resnet101_state(0) if arch == "resnet101" else synth.vgg16_state(0)
    d = 2048 if arch == "resnet101" else 512
    lin = synth.whitening_state(4, d)
    for key in ("lwhiten", "pool.whiten", "whiten"):              # one well-conditioned matrix for every layer: the timing does not depend on the values
        sd[key + ".weight"], sd[key + ".bias"] = torch.from_numpy(lin["P"]), torch.from_numpy(lin["m"]).reshape(-1)
    sd["pool.rpool.p"] = sd["pool.p"]
    nets = {name: engine.build_embedder(sd, dev, head=head) for name, head in CONFIGS}
    for net in nets.values():
        for _ in range(3):
            net.forward(x)
    torch.cuda.synchronize()
    t = {k: [] for k in nets}
    for _ in range(iters):                                        # alternating: all see the same clocks / neighbours
        for k, net in nets.items():
            t[k].append(timed(net, x))
    row = {}
    for k, net in nets.items():
        v = sorted(t[k])
        row[k] = {"ms_median": round(v[len(v) // 2], 3), "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3)}
        net.set_profiling(True)
        net.forward(x)
        torch.cuda.synchronize()
        p = net.profile()
        net.set_profiling(False)
        row[k]["head_op_ms"] = round(sum(ms for kind, _, ms, _ in p if kind in (OP_GEM, OP_POOL_HEAD)), 3)
        row[k]["last_conv_ms"] = round([ms for kind, _, ms, _ in p if kind == OP_CONV][-1], 3)      # the local whitening where there is one
        row[k]["last_conv_variant"] = [v for kind, v, _, _ in p if kind == OP_CONV][-1]
        row[k]["sum_of_ops_ms"] = round(sum(ms for _, _, ms, _ in p), 3)
        row[k]["head_launches"] = list(net.head_launches(*G))
    base = row["gem"]["ms_median"]
    for k in nets:
        row[k]["over_plain_gem"] = round(row[k]["ms_median"] / base, 4)
    out["archs"][arch] = row
    del nets
    torch.cuda.empty_cache()
print(json.dumps(out))
