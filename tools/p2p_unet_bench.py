"""dev tool: the normalisation U-Nets (p2p_unet, outconv_unet, inconv_p2p_unet, aligned_p2p_unet, shallow_p2p_unet; default nested_levels, synthetic weights) on
one device at 64 x 3 x 256^2 (the generators' geometry) and 4 x 3 x 1024^2 (the embedder's image size, where these nets are used).
Everything is compared inside this process, alternating, after a warm-up of every variant:
  * the whole forward of each net in f16 and in f16x3 -- event-timed;
  * for aligned_p2p_unet, the whole f16 forward with the concatenation conv on conv3x3_cat_halo.hip and with GDT_CONV3X3_CAT_HALO=0 (copy of the concatenation + the
    3x3 conv of one tensor), and that layer alone from the executor's per-op event profile (gdt_net_set_profiling; five profiled forwards per route, alternating,
    averaged): ms, run-to-run spread, algorithmic TFLOP/s;
  * the concatenation conv alone on other eligible shapes (``cat_conv_sweep``), both routes, the same way.
Event-timed single forwards leave idle gaps and run at higher clocks than a sustained run: they rank kernels; bench.py quotes speed.
Prints one JSON line and writes it to the path given (default profiles/p2p_unet_1gpu.json).
usage: tools/p2p_unet_bench.py [iters] [out.json]      (default 10 timed forwards per variant)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                     # noqa: E402

from gandtr_amd import engine                                    # noqa: E402
from gandtr_amd.components.model.network import unet             # noqa: E402
from gandtr_amd.tools import synth                               # noqa: E402

KNOB = "GDT_CONV3X3_CAT_HALO"
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 10
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "p2p_unet_1gpu.json")
dev = torch.device("cuda:0")
GEOMETRIES = ((64, 256, 256), (4, 1024, 1024))
ROUTES = {"cat_kernel": None, "generic": "0"}
SWEEP_ROUTES = {"cat_kernel": "2", "generic": "0"}           # (2: the kernel wherever it is eligible, also where the default routes the shape to the generic route)
# (cin_a, cin_b, cout, batch, side) of the concatenation conv alone: wider layers, unequal halves, several column tiles, maps with few patches
SWEEP = ((64, 64, 64, 4, 512), (64, 64, 64, 4, 128), (64, 64, 64, 1, 64), (128, 128, 128, 4, 512), (64, 128, 256, 4, 256), (256, 256, 256, 4, 256), (512, 512, 512, 4, 64),
         (512, 512, 512, 1, 16))


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


def stats(v, gflop, images):
    v = sorted(v)
    med = v[len(v) // 2]
    return {"ms_median": round(med, 3), "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3), "tflops": round(gflop / med, 1), "images_per_s": round(images / med * 1e3, 1)}


def profiled(net, x):
    net.set_profiling(True)
    net.forward(x)
    torch.cuda.synchronize()
    rows = net.profile()
    net.set_profiling(False)
    return rows


out = {"workload": "normalisation U-Nets (unet.py), default nested_levels, synthetic weights, forward", "iters": iters, "geometries": {}}
for G in GEOMETRIES:
    x = synth.synth_input(50, (G[0], 3, G[1], G[2]), 1.0).to(dev)
    grow = {}
    for label in unet.LABELS:
        cfg = unet.family_config(label, 3, 3)
        sd = synth.p2p_unet_state(label, 0)
        nets = {prec: engine.build_p2p_unet(label, sd, dev, cfg, precision=prec) for prec in ("f16", "f16x3")}
        aligned = label == "aligned_p2p_unet"
        routes = ROUTES if aligned else {"cat_kernel": None}
        for value in routes.values():                                # warm-up of every variant
            knob(value)
            for net in nets.values():
                for _ in range(2):
                    net.forward(x)
        knob(None)
        torch.cuda.synchronize()
        t = {k: [] for k in routes}
        tx = []
        for _ in range(iters):
            for k, value in routes.items():
                knob(value)
                t[k].append(timed(lambda: nets["f16"].forward(x)))
            knob(None)
            tx.append(timed(lambda: nets["f16x3"].forward(x)))
        gf = nets["f16"].flops(*G) / 1e9
        row = {"nested_levels": cfg["nested_levels"], "gflop_per_image": round(gf / G[0], 2), "f16": stats(t["cat_kernel"], gf, G[0]), "f16x3": stats(tx, gf, G[0]),
               "conv3x3_cat_launches": nets["f16"].conv3x3_cat_launches(*G), "conv4x4t_launches": nets["f16"].conv4x4t_launches(*G),
               "workspace_gb": {p: round(n.workspace_bytes(*G) / 1e9, 3) for p, n in nets.items()}}
        if aligned:
            row["f16_generic_route"] = stats(t["generic"], gf, G[0])
            row["forward_generic_over_kernel"] = round(row["f16_generic_route"]["ms_median"] / row["f16"]["ms_median"], 3)
            row["forward_spread_ms"] = {k: round(max(v) - min(v), 3) for k, v in t.items()}
            prof = {k: [] for k in ROUTES}
            for _ in range(5):
                for k, value in ROUTES.items():
                    knob(value)
                    prof[k].append(profiled(nets["f16"], x))
            knob(None)
            kinds = [r[0] for r in prof["generic"][0]]
            i = next(j for j in range(1, len(kinds)) if kinds[j] == 1 and kinds[j - 1] == 9 and any(908000 <= run[j][1] < 909000 for run in prof["cat_kernel"]))
            ms = lambda k, j: [run[j][2] for run in prof[k]]
            mean = lambda v: sum(v) / len(v)
            fl = prof["generic"][0][i][3]
            kern = [a + b for a, b in zip(ms("cat_kernel", i), ms("cat_kernel", i - 1))]          # (the copy op is skipped on this route: 0 ms)
            gen = [a + b for a, b in zip(ms("generic", i), ms("generic", i - 1))]
            row["cat_conv"] = {"cin_a": 64, "cin_b": 64, "cout": 64, "hw": [G[1], G[2]], "gflop": round(fl / 1e9, 2),
                               "kernel": {"variant": prof["cat_kernel"][0][i][1], "ms": round(mean(kern), 4), "spread_ms": round(max(kern) - min(kern), 4),
                                          "tflops": round(fl / 1e9 / mean(kern), 1)},
                               "generic": {"variant": prof["generic"][0][i][1], "ms": round(mean(gen), 4), "spread_ms": round(max(gen) - min(gen), 4),
                                           "copy_ms": round(mean(ms("generic", i - 1)), 4), "conv_ms": round(mean(ms("generic", i)), 4),
                                           "tflops": round(fl / 1e9 / mean(gen), 1)}}
            row["cat_conv"]["generic_over_kernel"] = round(mean(gen) / mean(kern), 3)
        grow[label] = row
        del nets
        torch.cuda.empty_cache()
    out["geometries"]["%dx3x%dx%d" % G] = grow

# ---- the concatenation conv alone on other eligible shapes: two 1x1 convs of the image feed it; per-op events, five profiled forwards per route, alternating
sweep = {}
for ca, cb, cout, n, side in SWEEP:
    net = engine.HipNet(dev, "f16")
    t = net.input(3)
    a = net.conv(t, synth._normal(1, "wa", (ca, 3, 1, 1), 0.7), relu=True)
    b = net.conv(t, synth._normal(1, "wb", (cb, 3, 1, 1), 0.7), relu=True)
    net.out_slot = net.output_nchw(net.conv_cat(a, b, synth._normal(2, "wc", (cout, ca + cb, 3, 3), (2.0 / (9 * (ca + cb))) ** 0.5), pad=1, relu=True))
    net.finalize()
    x = synth.synth_input(51, (n, 3, side, side), 1.0).to(dev)
    prof = {k: [] for k in ROUTES}
    default_route = "cat_kernel" if net.conv3x3_cat_launches(n, side, side) else "generic"                # (knob unset: the routing rule of the kernel file)
    for rep in range(7):
        for k, value in SWEEP_ROUTES.items():
            knob(value)
            rows = profiled(net, x)
            if rep >= 2:                                              # (two warm-up rounds)
                prof[k].append(rows)
    knob(None)
    kinds = [r[0] for r in prof["generic"][0]]
    i = next(j for j in range(1, len(kinds)) if kinds[j] == 1 and kinds[j - 1] == 9)
    fl = prof["generic"][0][i][3]
    entry = {"gflop": round(fl / 1e9, 2), "default_route": default_route, "patches_x_column_tiles": n * ((side + 7) // 8) * ((side + 15) // 16) * (cout // 64)}
    for k in ROUTES:
        v = [run[i][2] + run[i - 1][2] for run in prof[k]]
        m = sum(v) / len(v)
        entry[k] = {"variant": prof[k][0][i][1], "ms": round(m, 4), "spread_ms": round(max(v) - min(v), 4), "tflops": round(fl / 1e9 / m, 1)}
    entry["generic_over_kernel"] = round(entry["generic"]["ms"] / entry["cat_kernel"]["ms"], 3)
    sweep["%d+%d->%d@%dx%d^2" % (ca, cb, cout, n, side)] = entry
    del net
    torch.cuda.empty_cache()
out["cat_conv_sweep"] = sweep

line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
