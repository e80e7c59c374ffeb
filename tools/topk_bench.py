"""Cost of the streaming top-k, of query expansion and of database augmentation next to the routes the repository had before, on the same GPU.

python tools/topk_bench.py [--json profiles/topk_qe_1gpu.json] [--reps 5] [--baseline-reps 2] [--sizes full]
  top-k shapes (ndb x nq, d, k), random unit vectors made on the device from a seed:
    topk            retrieval.topk (gdt_retrieval_topk: scan + merge, f32-input MFMAs, no score matrix);
    sort_then_slice retrieval.scores_and_ranks(with_ranks=True) and the first k rows of the ranks: the earlier route to the same answer;
    scores_only     retrieval.scores_and_ranks(with_ranks=False): the f16x3 GEMM alone, i.e. what the products cost in the other arithmetic.
  The three alternate inside one process; device events around each call, the first round left out as warm-up, median / min / max of --reps.
  DBA shape (n vectors, d, k):
    augment_database  retrieval.augment_database (top-k of the database against itself in blocks, then gdt_retrieval_expand);
    torch_blocks      torch.mm + torch.topk over query blocks, then the same weighted sum and l2n in torch ops;
    scores_only       the f16x3 scores GEMM of ONE block of queries against the database, as the rate to hold the achieved FLOP/s against.
  Also recorded: how many of topk's ids equal the sorted route's, and the largest share of tests/test_hip_topk.py's rounding gate that
  gdt_retrieval_expand reaches on that test's cases (tests/topk_ref.py is the float64 oracle)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gandtr_amd import retrieval                                            # noqa: E402

SIZES = {"full": {"topk": [(200000, 70, 2048, 100), (20000, 2000, 2048, 100)], "dba": (200000, 512, 10, 8192, 2048)},
         "small": {"topk": [(20000, 70, 256, 100)], "dba": (20000, 64, 10, 8192, 2048)}}


def unit_rows(seed, n, d, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    v = torch.randn((n, d), generator=g, device=dev, dtype=torch.float32)
    return v / v.norm(dim=1, keepdim=True)


def timed_round_robin(fns, reps):
    """fns: name -> callable.  One warm-up round, then `reps` rounds in which the callables alternate."""
    ms = {name: [] for name in fns}
    out = {}
    for r in range(reps + 1):
        for name, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            out[name] = fn()
            e.record()
            torch.cuda.synchronize()
            if r:
                ms[name].append(s.elapsed_time(e))
    return out, {name: {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                        "runs_ms": [round(x, 3) for x in v]} for name, v in ms.items()}


def topk_record(ndb, nq, d, k, reps, dev):
    v, q = unit_rows(1, ndb, d, dev), unit_rows(2, nq, d, dev)
    V, Q = v.t(), q.t()                                                     # D x N views of row-major blocks: no copy inside the calls

    def sort_then_slice():
        scores, ranks = retrieval.scores_and_ranks(V, Q, with_ranks=True)
        return ranks[:k].contiguous()

    fns = {"topk": lambda: retrieval.topk(V, Q, k), "sort_then_slice": sort_then_slice,
           "scores_only": lambda: retrieval.scores_and_ranks(V, Q, with_ranks=False)[0]}
    out, t = timed_round_robin(fns, reps)
    ids = out["topk"][1]
    flops = 2.0 * ndb * nq * d
    spread = max(t[n]["max_ms"] - t[n]["min_ms"] for n in ("topk", "sort_then_slice"))
    rec = {"shape": {"ndb": ndb, "nq": nq, "d": d, "k": k}, "times": t,
           "ids_equal_to_sorted_route": round(float((ids == out["sort_then_slice"]).float().mean()), 6),
           "topk_TFLOPs_fp32": round(flops / (t["topk"]["median_ms"] * 1e-3) / 1e12, 2),
           "scores_only_TFLOPs_products": round(flops / (t["scores_only"]["median_ms"] * 1e-3) / 1e12, 2),
           "topk_over_sort_then_slice": round(t["topk"]["median_ms"] / t["sort_then_slice"]["median_ms"], 3),
           "topk_over_scores_only": round(t["topk"]["median_ms"] / t["scores_only"]["median_ms"], 3),
           "largest_spread_ms": round(spread, 3),
           "topk_faster_than_sort_then_slice_beyond_spread": bool(t["sort_then_slice"]["median_ms"] - t["topk"]["median_ms"] > spread)}
    del v, q, out
    torch.cuda.empty_cache()
    return rec


def torch_dba(v, k, alpha, block):
    out = torch.empty_like(v)
    for b0 in range(0, v.shape[0], block):
        q = v[b0:b0 + block]
        s, i = torch.topk(torch.mm(q, v.t()), k, dim=1)
        w = s.clamp_min(0).pow(alpha) if alpha else torch.ones_like(s)
        x = (w[:, :, None] * v[i]).sum(1)
        out[b0:b0 + block] = x / (x.norm(dim=1, keepdim=True) + 1e-6)
    return out


def dba_record(n, d, k, block, torch_block, reps, baseline_reps, dev):
    v = unit_rows(3, n, d, dev)
    V = v.t()
    out, t = timed_round_robin({"augment_database": lambda: retrieval.augment_database(V, k, 3.0, block)}, reps)
    base, tb = timed_round_robin({"torch_blocks": lambda: torch_dba(v, k, 3.0, torch_block)}, baseline_reps)
    nq = min(block, n)
    _, tg = timed_round_robin({"scores_only": lambda: retrieval.scores_and_ranks(V, v[:nq].t(), with_ranks=False)[0]}, reps)
    got, ref = out["augment_database"].t(), base["torch_blocks"]
    flops = 2.0 * n * n * d
    rec = {"shape": {"n": n, "d": d, "k": k, "alpha": 3.0, "block": block, "torch_block": torch_block},
           "times": {**t, **tb, "scores_only_one_block": tg["scores_only"]},
           "augment_database_TFLOPs_fp32": round(flops / (t["augment_database"]["median_ms"] * 1e-3) / 1e12, 2),
           "scores_only_one_block_TFLOPs_products": round(2.0 * n * nq * d / (tg["scores_only"]["median_ms"] * 1e-3) / 1e12, 2),
           "augment_database_over_torch_blocks": round(t["augment_database"]["median_ms"] / tb["torch_blocks"]["median_ms"], 3),
           "min_cosine_to_torch_blocks": round(float((got * ref).sum(1).min()), 7)}
    return rec


def expand_gate_share(dev):
    """the cases of tests/test_hip_topk.py::test_expand_matches_float64_under_the_rounding_gate without holes: err / gate, largest"""
    import topk_ref as R
    worst = 0.0
    for d in (7, 512):
        v, q = unit_rows(4, 400, d, dev), unit_rows(5, 6, d, dev)
        for k in (1, 10):
            scores, ids = retrieval._topk_rows(v, q, k)
            for alpha in (0.0, 1.0, 3.0):
                for base in (q, None):
                    out = retrieval._expand_rows(v, base, ids, scores, alpha)
                    ref, mag, norm = R.ref_expand(v.cpu().numpy(), None if base is None else q.cpu().numpy(), ids.cpu().numpy(),
                                                  scores.cpu().numpy(), alpha)
                    gate = (k + 8) * 2.0 ** -23 * mag / norm
                    worst = max(worst, float((np.abs(out.cpu().numpy().astype(np.float64) - ref) / gate).max()))
    return round(worst, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="full", choices=sorted(SIZES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-reps", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_bench measures on a GPU; none found")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "tool": "tools/topk_bench.py", "reps": a.reps,
              "arithmetic": "topk: v_mfma_f32_32x32x2_f32 on fp32 operands; scores_only / sort_then_slice: f16x3 GEMM", "topk": []}
    for ndb, nq, d, k in SIZES[a.sizes]["topk"]:
        rec = topk_record(ndb, nq, d, k, a.reps, dev)
        print(json.dumps(rec), flush=True)
        result["topk"].append(rec)
    result["expand_largest_share_of_rounding_gate"] = expand_gate_share(dev)
    print(json.dumps({"expand_largest_share_of_rounding_gate": result["expand_largest_share_of_rounding_gate"]}), flush=True)
    n, d, k, block, torch_block = SIZES[a.sizes]["dba"]
    result["dba"] = dba_record(n, d, k, block, torch_block, a.reps, a.baseline_reps, dev)
    print(json.dumps(result["dba"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
