"""dev: build one of the models with synthetic weights on cuda:0 and probe its forward at the given shapes, from the executor's own per-op event profile
(HipNet.set_profiling / profile) or by wall time.

usage: tools/net_probe.py MODEL [--precision P] --shape N,H,W [--shape ...] MODE [options]

  MODEL  gen | genbn (ResnetGenerator, InstanceNorm / BatchNorm) | disc | discbn (NLayerDiscriminator, likewise) | hed | rcf | r101 | vgg16 (GeM embedders)
  MODE   ops       per-op table of one profiled forward: index, kind, kernel variant, ms, TFLOP/s (--bytes: and GB/s of the algorithmic HBM bytes);
                   --min-ms T shows the ops of at least T ms, --from-op I those from index I on; the total counts every op
         variants  the same forward summed by (kind, variant), largest first
         mean5     five profiled forwards averaged, one line per op in the format tools/agg.py reads
         time      wall time of --steps forwards after --warmup (synchronised at both ends): ms, items/s, ns/pixel

Event-timed tables leave idle gaps between kernels and run at higher clocks than a sustained run: compare kernels with them, quote speed from bench.py.

This tool replaces one script per model and shape list.  Their command lines, with the shapes and thresholds they had:

  r101_ops.py        r101 --shape 32,1024,1024 ops --min-ms 0.25          (it also listed every op below index 40)
  r101_tail_ops.py   r101 --shape 32,1024,1024 ops --bytes --from-op 95 --min-ms 0.01
  r101_ops_small.py  r101 --shape 1,1024,1024 --shape 8,512,512 --shape 8,724,724 --shape 128,256,256 --shape 32,1024,683 variants      (it cut at 14 rows)
  vgg16_ops.py       vgg16 --shape 32,1024,1024 ops --min-ms 0.05
  vgg16_ragged.py    vgg16 --shape 32,1024,683 --shape 32,1024,768 time --steps 5      and the same shapes with: ops --min-ms 0.2
  gen_ops.py         gen --shape 64,256,256 ops
  gen_bn_ops.py      genbn --shape 64,256,256 ops
  hed_ops.py         hed --shape 64,256,256 ops --min-ms 0.02
  dump_ops.py        M --precision f16 --shape S mean5      with (M, S) = (gen | genbn | hed, 64,256,256), (r101, 32,1024,1024), (vgg16, 8,1024,1024)
  r101_small.py      r101 --shape 128,256,256 --shape 8,512,512 --shape 8,1024,1024 --shape 1,1024,1024 --shape 4,724,724 time
  r101_sizes.py      r101 --shape 32,1024,1024 --shape 32,724,724 --shape 32,512,512 --shape 32,1024,768 --shape 32,1024,683 --shape 16,1024,1024
                          --shape 24,1024,1024 time      (run twice: GDT_CONV_XEXP=0 / 1)
  r101_ragged.py     r101 --shape 32,1024,683 --shape 32,1024,768 --shape 16,1000,1000 time --steps 6
  batch_small.py     gen --precision P --shape 1,256,256 --shape 2,256,256 --shape 4,256,256 --shape 8,256,256 --shape 16,256,256 --shape 1,1024,1024
                          time --steps 30 --warmup 5      for P in f16c, f16, f16x3
"""
import argparse
import collections
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                     # noqa: E402

from gandtr_amd import engine                                    # noqa: E402
from gandtr_amd.tools import synth                               # noqa: E402

KINDS = ("input", "conv", "inorm", "maxpool", "gem", "tap", "hed", "rcf", "poolhead")      # OpKind, csrc/net_internal.h
CAFFE_INPUT = dict(perm=[2, 1, 0], in_affine=([255.0] * 3, [-104.0, -117.0, -123.0]))      # RgbToBgrPre + MeanStdPre folded into the input pack


def build(model, dev, precision):
    """(net, clamp of its synthetic input): the generators and edge detectors read images in [-1, 1], the embedders normalised ones"""
    kw = {} if precision is None else {"precision": precision}      # None: the builder's own default (generator f16c, the others f16)
    if model in ("gen", "genbn"):
        return engine.build_generator(synth.generator_state(0, "instance" if model == "gen" else "batch"), dev, **kw), 1.0
    if model in ("disc", "discbn"):
        return engine.build_discriminator(synth.discriminator_state(0, "instance" if model == "disc" else "batch", gain=0.2 if model == "disc" else None), dev, **kw), 1.0
    if model == "hed":
        return engine.build_hed(synth.hed_state(0), dev, **CAFFE_INPUT, **kw), 1.0
    if model == "rcf":
        return engine.build_rcf(synth.rcf_state(0), dev, **CAFFE_INPUT, **kw), 1.0
    return engine.build_embedder(synth.resnet101_state(0) if model == "r101" else synth.vgg16_state(0), dev, **kw), None


def profiled(net, x):
    """(rows of profile(), algorithmic bytes per op) of one forward"""
    net.set_profiling(True)
    net.forward(x)
    torch.cuda.synchronize()
    rows, by = net.profile(), net.profile_bytes()
    net.set_profiling(False)
    return rows, by


def rate(amount, ms, unit):
    return amount / ms / unit if ms > 0 else 0.0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter,
                                 epilog="the module docstring lists the command lines of the scripts this tool replaced")
    ap.add_argument("model", choices=("gen", "genbn", "disc", "discbn", "hed", "rcf", "r101", "vgg16"))
    ap.add_argument("mode", choices=("ops", "variants", "mean5", "time"))
    ap.add_argument("--precision", choices=sorted(engine.HipNet.PRECISIONS), default=None, help="default: the builder's own")
    ap.add_argument("--shape", action="append", required=True, metavar="N,H,W", help="batch, height, width; may be given several times")
    ap.add_argument("--min-ms", type=float, default=0.0, help="ops / variants: rows of at least this many ms")
    ap.add_argument("--from-op", type=int, default=0, help="ops: rows from this op index on")
    ap.add_argument("--bytes", action="store_true", help="ops: add the GB/s column")
    ap.add_argument("--steps", type=int, default=10, help="time: timed forwards")
    ap.add_argument("--warmup", type=int, default=3, help="forwards before anything is measured")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shape]
    if any(len(s) != 3 or min(s) < 1 for s in shapes):
        ap.error("--shape takes N,H,W")
    dev = torch.device("cuda:0")
    net, clamp = build(a.model, dev, a.precision)
    for n, h, w in shapes:
        x = synth.synth_input(1, (n, 3, h, w), clamp).to(dev)
        for _ in range(a.warmup):
            net.forward(x)
        torch.cuda.synchronize()
        if len(shapes) > 1:
            print("%s %s %d x 3 x %d x %d" % (a.model, net.precision, n, h, w))
        if a.mode == "time":
            t0 = time.perf_counter()
            for _ in range(a.steps):
                net.forward(x)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / a.steps
            print("%d x 3 x %d x %d  %.3f ms  %.0f items/s  %.2f ns/pixel" % (n, h, w, dt * 1e3, n / dt, dt * 1e9 / (n * h * w)))
        elif a.mode == "mean5":
            runs = [profiled(net, x)[0] for _ in range(5)]
            ms = [sum(r[i][2] for r in runs) / 5 for i in range(len(runs[0]))]
            tot = sum(ms)
            for i, ((kind, variant, _, fl), m) in enumerate(zip(runs[0], ms)):
                print("%3d %-8s var %6d  %8.3f ms  %6.1f%%  %8.2f GFLOP  %7.1f TFLOP/s" % (i, KINDS[kind], variant, m, 100 * m / tot, fl / 1e9, rate(fl, m, 1e9)))
            print("total %.3f ms" % tot)
        else:
            rows, by = profiled(net, x)
            if a.mode == "ops":
                for i, ((kind, variant, ms, fl), b) in enumerate(zip(rows, by)):
                    if i >= a.from_op and ms >= a.min_ms:
                        print("%3d kind %d variant %7d  %7.3f ms  %7.1f TF" % (i, kind, variant, ms, rate(fl, ms, 1e9))
                              + ("  %7.1f GB/s" % rate(b, ms, 1e6) if a.bytes else ""))
            else:
                acc = collections.OrderedDict()
                for kind, variant, ms, fl in rows:
                    e = acc.setdefault((kind, variant), [0, 0.0, 0.0])
                    e[0] += 1; e[1] += ms; e[2] += fl
                for (kind, variant), (count, ms, fl) in sorted(acc.items(), key=lambda kv: -kv[1][1]):
                    if ms >= a.min_ms:
                        print("   kind %d variant %7d  x%3d  %6.3f ms  %6.1f TF" % (kind, variant, count, ms, rate(fl, ms, 1e9)))
            print("total %.3f ms" % sum(r[2] for r in rows))


if __name__ == "__main__":
    main()
