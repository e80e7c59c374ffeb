"""Cost of the device mAP evaluation next to the sort that precedes it and the host evaluation it replaces.

python tools/map_bench.py --ndb 100000 [--nq 70] [--dim 128] [--reps 5] [--json OUT]
  scores_and_ranks (f16x3 GEMM + segmented radix sort) on random unit descriptors, then compute_map_and_print on those ranks -- three
  setups (easy / medium / hard, roxford5k-sized ground truth: ~50 easy, ~50 hard, ~100 junk per query) in one average-precision launch
  chain -- timed with device events; and the numpy compute_map_and_print on the same ranks (host wall time).  The kernel-level split
  (sort vs AP launches) comes from running this under ``rocprofv3 --kernel-trace --stats`` in a run of its own."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gandtr_amd import retrieval                                            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndb", type=int, required=True)
    ap.add_argument("--nq", type=int, default=70)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host", type=int, default=1, help="also time the numpy evaluation (0: skip)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    vecs = torch.nn.functional.normalize(torch.randn((a.dim, a.ndb), device=dev, generator=g), dim=0)
    qvecs = torch.nn.functional.normalize(torch.randn((a.dim, a.nq), device=dev, generator=g), dim=0)
    rng = np.random.default_rng(0)
    gnd = [{"easy": rng.choice(a.ndb, 50, replace=False).tolist(), "hard": rng.choice(a.ndb, 50, replace=False).tolist(),
            "junk": rng.choice(a.ndb, 100, replace=False).tolist()} for _ in range(a.nq)]
    sink = io.StringIO()

    def timed(fn):
        ms = []
        for _ in range(a.reps + 1):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            out = fn()
            e.record()
            torch.cuda.synchronize()
            ms.append(s.elapsed_time(e))
        return out, float(np.median(ms[1:]))

    (_, ranks), rank_ms = timed(lambda: retrieval.scores_and_ranks(vecs, qvecs))
    with contextlib.redirect_stdout(sink):
        dev_out, map_ms = timed(lambda: retrieval.compute_map_and_print("roxford5k", ranks, gnd))
    res = {"ndb": a.ndb, "nq": a.nq, "setups": 3, "scores_and_ranks_ms": round(rank_ms, 3), "device_compute_map_and_print_ms": round(map_ms, 3)}
    if a.host:
        host = ranks.cpu().numpy().astype(np.int64)
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(sink):
            host_out = retrieval.compute_map_and_print("roxford5k", host, gnd)
        res["host_compute_map_and_print_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["same_as_host"] = all(dev_out[0][k] == host_out[0][k] for k in dev_out[0])
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
