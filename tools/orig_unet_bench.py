"""dev tool: ``orig_unet`` and ``outconv_dynint_unet`` (default arguments, synthetic weights) on one device at 4 x 3 x 1024^2 (the embedder's image size, where
these nets are used) and 64 x 3 x 256^2 (the generators' geometry).  Everything is compared inside this process, alternating, after a warm-up of every
variant; every figure is the median of 5 with min .. max:
  * per ConvTranspose2d(k2, s2) layer of orig_unet (f16): convt2x2.hip against this build's generic route (GDT_CONVT2X2=0: four phase launches), from the
    executor's per-op event profile (gdt_net_set_profiling), and the same op in torch (F.conv_transpose2d, fp16 channels-last) on the same GPU; TB/s of
    input + output + weight bytes;
  * the resize kernel alone (the net's outermost resize: 64 channels, H / 2 -> H) in fp16 and fp32 against F.interpolate;
  * the whole forwards: both nets, both geometries, f16 and f16x3 (orig_unet f16 on both routes of its transposed convs).
Event-timed single forwards leave idle gaps and run at higher clocks than a sustained run: they rank kernels; bench.py quotes speed.
Prints one JSON line and writes it to the path given (default profiles/orig_unet_1gpu.json).
usage: tools/orig_unet_bench.py [out.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                     # noqa: E402
import torch.nn.functional as F                                  # noqa: E402

from gandtr_amd import engine                                    # noqa: E402
from gandtr_amd.components.model.network import unet             # noqa: E402
from gandtr_amd.tools import synth                               # noqa: E402

KNOB = "GDT_CONVT2X2"
REPS = 5
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "orig_unet_1gpu.json")
dev = torch.device("cuda:0")
GEOMETRIES = ((4, 1024, 1024), (64, 256, 256))
ROUTES = {"convt2x2": None, "generic": "0"}


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


out = {"workload": "orig_unet / outconv_dynint_unet (unet.py), default arguments, synthetic weights, forward; medians of %d with min .. max" % REPS, "geometries": {}}
orig_cfg = dict(in_channels=3, out_channels=3, nested_levels=4, min_channels=64)
orig_sd = synth.orig_unet_state(0)
dyn = unet.OutconvP2pUNetDynamicInterpolate(3, 3)
dyn_sd = synth.dynint_unet_state(0)
for G in GEOMETRIES:
    n, h, w = G
    x = synth.synth_input(50, (n, 3, h, w), 1.0).to(dev)
    grow = {}
    # ---- orig_unet: whole forwards, and the transposed convs one by one
    nets = {prec: engine.build_orig_unet(orig_sd, dev, orig_cfg, precision=prec) for prec in ("f16", "f16x3")}
    for value in ROUTES.values():
        knob(value)
        for net in nets.values():
            for _ in range(2):
                net.forward(x)
    knob(None)
    torch.cuda.synchronize()
    t = {k: [] for k in ROUTES}
    tx = []
    for _ in range(REPS):
        for k, value in ROUTES.items():
            knob(value)
            t[k].append(timed(lambda: nets["f16"].forward(x)))
        knob(None)
        tx.append(timed(lambda: nets["f16x3"].forward(x)))
    gf = nets["f16"].flops(*G) / 1e9
    row = {"gflop": round(gf, 1), "f16": med(t["convt2x2"], 3), "f16_generic_route": med(t["generic"], 3), "f16x3": med(tx, 3),
           "plan": {k: v for k, v in nets["f16"].plan_summary(*G).items() if v}, "workspace_gb": {p: round(net.workspace_bytes(*G) / 1e9, 3) for p, net in nets.items()}}
    prof = {k: [] for k in ROUTES}
    for _ in range(REPS):
        for k, value in ROUTES.items():
            knob(value)
            prof[k].append(profiled(nets["f16"], x))
    knob(None)
    layers = {}
    ups = [j for j, r in enumerate(prof["convt2x2"][0]) if r[0] == 1 and r[1] == 902128]
    for depth, j in enumerate(ups):                                   # (the innermost transposed conv runs first)
        level = len(ups) - 1 - depth
        cout = 64 * 2 ** level
        cin, hh, ww = 2 * cout, h >> (level + 1), w >> (level + 1)
        nbytes = 2.0 * n * hh * ww * cin + 2.0 * n * 4 * hh * ww * cout + 2.0 * cin * cout * 4
        entry = {"cin": cin, "cout": cout, "in_hw": [hh, ww], "gflop": round(prof["convt2x2"][0][j][3] / 1e9, 2), "mbytes": round(nbytes / 1e6, 1)}
        for k in ROUTES:
            entry[k] = dict(med([run[j][2] for run in prof[k]]), variant=prof[k][0][j][1])
            entry[k]["tb_per_s"] = round(nbytes / entry[k]["ms"] / 1e9, 2)
        xt = torch.randn(n, cin, hh, ww, device=dev, dtype=torch.float16).contiguous(memory_format=torch.channels_last)
        wt = (torch.randn(cin, cout, 2, 2, device=dev) * (2.0 / cin) ** 0.5).half()
        bt = torch.zeros(cout, device=dev, dtype=torch.float16)
        for _ in range(2):
            F.conv_transpose2d(xt, wt, bt, stride=2)
        entry["torch"] = med([timed(lambda: F.conv_transpose2d(xt, wt, bt, stride=2)) for _ in range(REPS)])
        entry["torch"]["tb_per_s"] = round(nbytes / entry["torch"]["ms"] / 1e9, 2)
        entry["generic_over_kernel"] = round(entry["generic"]["ms"] / entry["convt2x2"]["ms"], 3)
        entry["torch_over_kernel"] = round(entry["torch"]["ms"] / entry["convt2x2"]["ms"], 3)
        layers["%d->%d@%dx%dx%d" % (cin, cout, n, hh, ww)] = entry
        del xt, wt
    row["transposed_layers"] = layers
    grow["orig_unet"] = row
    del nets
    torch.cuda.empty_cache()
    # ---- outconv_dynint_unet: whole forwards
    nets = {prec: engine.build_dynint_unet(dyn_sd, dev, dyn._cfg, precision=prec) for prec in ("f16", "f16x3")}
    for net in nets.values():
        for _ in range(2):
            net.forward(x)
    torch.cuda.synchronize()
    t16, t3 = [], []
    for _ in range(REPS):
        t16.append(timed(lambda: nets["f16"].forward(x)))
        t3.append(timed(lambda: nets["f16x3"].forward(x)))
    rows = [profiled(nets["f16"], x) for _ in range(REPS)]
    resize_ops = [j for j, r in enumerate(rows[0]) if r[0] == 11]
    grow["outconv_dynint_unet"] = {"gflop": round(nets["f16"].flops(*G) / 1e9, 1), "f16": med(t16, 3), "f16x3": med(t3, 3),
                                   "plan": {k: v for k, v in nets["f16"].plan_summary(*G).items() if v},
                                   "resize_ops": len(resize_ops), "resize_ms_total_f16": med([sum(run[j][2] for j in resize_ops) for run in rows]),
                                   "workspace_gb": {p: round(net.workspace_bytes(*G) / 1e9, 3) for p, net in nets.items()}}
    del nets
    torch.cuda.empty_cache()
    # ---- the resize kernel alone: 64 channels, H / 2 -> H (the net's outermost resize, one of its two tensors), against F.interpolate
    rrow = {}
    for prec, dtype in (("f16", torch.float16), ("f16x3", torch.float32)):
        net = engine.HipNet(dev, prec)
        like = net.conv(net.input(3), synth._normal(1, "wa", (8, 3, 1, 1), 0.7))
        small = net.conv(like, synth._normal(1, "wb", (64, 8, 4, 4), 0.1), stride=2, pad=1)
        net.out_slot = net.output_nchw(net.conv(net.resize(small, like, "bilinear"), synth._normal(1, "wc", (8, 64, 1, 1), 0.1)))
        net.finalize()
        for _ in range(2):
            net.forward(x)
        runs = [profiled(net, x) for _ in range(REPS)]
        j = next(i for i, r in enumerate(runs[0]) if r[0] == 11)
        es = 2 if prec == "f16" else 4
        nbytes = float(es) * n * 64 * ((h // 2) * (w // 2) + h * w)
        xt = torch.randn(n, 64, h // 2, w // 2, device=dev, dtype=dtype).contiguous(memory_format=torch.channels_last)
        for _ in range(2):
            F.interpolate(xt, size=(h, w), mode="bilinear", align_corners=False)
        entry = {"kernel": med([run[j][2] for run in runs]), "torch": med([timed(lambda: F.interpolate(xt, size=(h, w), mode="bilinear", align_corners=False)) for _ in range(REPS)]),
                 "mbytes": round(nbytes / 1e6, 1)}
        entry["kernel"]["tb_per_s"] = round(nbytes / entry["kernel"]["ms"] / 1e9, 2)
        entry["torch"]["tb_per_s"] = round(nbytes / entry["torch"]["ms"] / 1e9, 2)
        entry["torch_over_kernel"] = round(entry["torch"]["ms"] / entry["kernel"]["ms"], 3)
        rrow[prec] = entry
        del net, xt
        torch.cuda.empty_cache()
    grow["resize_64ch_half_to_full"] = rrow
    out["geometries"]["%dx3x%dx%d" % G] = grow

line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
