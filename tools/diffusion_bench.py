"""Cost of diffusion re-ranking (gandtr_amd/csrc/retrieval_diffusion.hip) stage by stage, next to the same solver in torch ops on the same GPU.

python tools/diffusion_bench.py [--json profiles/diffusion_1gpu.json] [--reps 5] [--sizes full]
  Per shape (n database vectors, nq queries, d, k, kq), clustered unit vectors made on the device from a seed:
    graph      retrieval.knn_graph (the streaming top-k of the database against itself);
    affinity   retrieval.mutual_knn_affinity;
    seeds      retrieval.topk(vecs, qvecs, kq) and the seed weights;
    solve      retrieval.diffuse (conjugate gradients, alpha 0.99, tol 1e-5, at most 64 iterations);
    ranking    retrieval.rank_scores of the n x nq scores.
  Device events around each call, one warm-up round first, median / min / max of --reps (the graph build: --graph-reps).
  torch_cg: the same conjugate gradients written in torch ops -- a CSR torch.sparse.mm per iteration on the whole n x nq block, float64 dot
  products, a fixed number of iterations = the largest count the device solver reports -- alternating with `solve` inside one process.
  iteration: retrieval.diffuse with tol so small that no column stops, at 8 and at 24 iterations; the difference over 16 is one full iteration of a
  column block (all five launches), and the bytes its gathers read (valid neighbour ids x block width x 4) over that time is the gather rate with
  rows of `block` x 4 bytes -- a lower bound for the gather kernel itself, whose share of the iteration a kernel trace gives:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/diffusion_bench.py --trace
  runs nothing but one column block of 64 queries at n = 200000, k = 50 for 24 full iterations, three times (profiles/diffusion_kernel_stats.csv)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gandtr_amd import retrieval                                            # noqa: E402

GAMMA, ALPHA, TOL, MAX_ITER = 3.0, 0.99, 1e-5, 64
SIZES = {"full": [(4993, 70, 2048, 50, 10), (200000, 70, 512, 50, 10), (200000, 2000, 512, 50, 10)],
         "small": [(4993, 70, 256, 20, 10)]}


def clustered_rows(seed, n, d, per_cluster, noise, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    nc = max(n // per_cluster, 1)
    c = torch.randn((nc, d), generator=g, device=dev)
    c = c / c.norm(dim=1, keepdim=True)
    e = torch.randn((n, d), generator=g, device=dev)
    v = c[torch.randint(0, nc, (n,), generator=g, device=dev)] + noise * e / e.norm(dim=1, keepdim=True)
    return v / v.norm(dim=1, keepdim=True), c


def stats(v):
    return {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "runs_ms": [round(x, 3) for x in v]}


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
    return out, {name: stats(v) for name, v in ms.items()}


def torch_cg(S, y, alpha, iterations):
    """f, y: [n][nq] fp32; S: CSR fp32.  Plain conjugate gradients, every column `iterations` steps, dot products summed in float64."""
    x = torch.zeros_like(y)
    r = y.clone()
    p = y.clone()
    rr = (r * r).sum(0, dtype=torch.float64)
    for _ in range(iterations):
        ap = p - alpha * torch.sparse.mm(S, p)
        pap = (p * ap).sum(0, dtype=torch.float64)
        a = torch.where(pap > 0, rr / pap, torch.zeros_like(rr)).float()
        x += a * p
        r -= a * ap
        rr_new = (r * r).sum(0, dtype=torch.float64)
        b = torch.where(rr > 0, rr_new / rr, torch.zeros_like(rr)).float()
        p = r + b * p
        rr = rr_new
    return x


def shape_record(n, nq, d, k, kq, reps, graph_reps, dev, cache):
    key = (n, d, k)
    if key not in cache:
        cache.clear()
        v, centres = clustered_rows(1, n, d, 25, 0.6, dev)
        out, t = timed_round_robin({"graph": lambda: retrieval.knn_graph(v.t(), k)}, graph_reps)
        sc, ids = out["graph"]
        out, ta = timed_round_robin({"affinity": lambda: retrieval.mutual_knn_affinity(sc, ids, GAMMA)}, reps)
        cache[key] = (v, centres, sc, ids, out["affinity"], t["graph"], ta["affinity"])
    v, centres, sc, ids, w, t_graph, t_aff = cache[key]
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    e = torch.randn((nq, d), generator=g, device=dev)
    q = centres[torch.randint(0, centres.shape[0], (nq,), generator=g, device=dev)] + 0.6 * e / e.norm(dim=1, keepdim=True)
    q = q / q.norm(dim=1, keepdim=True)

    def seeds():
        s, sid = retrieval.topk(v.t(), q.t(), kq)
        return sid, s.clamp_min(0).pow(GAMMA)

    out, t_seeds = timed_round_robin({"seeds": seeds}, reps)
    sid, sw = out["seeds"]
    first = retrieval.diffuse(w, ids, sid, sw, ALPHA, TOL, MAX_ITER)
    iters = int(first.iterations.max())
    # the torch route's operands, built outside the timed window: CSR of the valid entries, y as a dense block
    idr, wr = ids.t().contiguous(), w.t().contiguous()
    valid = (idr >= 0) & (idr < n)
    crow = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    crow[1:] = valid.sum(1).cumsum(0)
    routes = {"solve": lambda: retrieval.diffuse(w, ids, sid, sw, ALPHA, TOL, MAX_ITER)}
    torch_error = None
    try:
        S = torch.sparse_csr_tensor(crow, idr[valid].long(), wr[valid], size=(n, n))
        y = torch.zeros((n, nq), dtype=torch.float32, device=dev)
        sv = (sid >= 0) & (sid < n)
        y.index_put_((sid.long().clamp(0, n - 1).reshape(-1), torch.arange(nq, device=dev).repeat(sid.shape[0])), (sw * sv).reshape(-1),
                     accumulate=True)
        torch_cg(S, y, ALPHA, 1)
        routes["torch_cg"] = lambda: torch_cg(S, y, ALPHA, iters)
    except Exception as ex:                                                 # recorded, not replaced by anything
        torch_error = "%s: %s" % (type(ex).__name__, ex)
    out, t_solve = timed_round_robin(routes, reps)
    res = out["solve"]
    _, t_rank = timed_round_robin({"ranking": lambda: retrieval.rank_scores(res.scores)}, reps)
    tiny = 1e-30
    _, t_it = timed_round_robin({"iters_8": lambda: retrieval.diffuse(w, ids, sid, sw, ALPHA, tiny, 8),
                                 "iters_24": lambda: retrieval.diffuse(w, ids, sid, sw, ALPHA, tiny, 24)}, reps)
    blocks = [(min(64, nq - q0)) for q0 in range(0, nq, 64)]
    widths = [1 << int(np.ceil(np.log2(b))) for b in blocks]
    gathered = float(valid.sum()) * 4.0 * sum(widths)                       # bytes the gathers of ONE iteration over all column blocks read
    it_ms = (t_it["iters_24"]["median_ms"] - t_it["iters_8"]["median_ms"]) / 16.0
    rec = {"shape": {"n": n, "nq": nq, "d": d, "k": k, "kq": kq, "gamma": GAMMA, "alpha": ALPHA, "tol": TOL, "max_iter": MAX_ITER},
           "times": {"graph": t_graph, "affinity": t_aff, "seeds": t_seeds["seeds"], **t_solve, "ranking": t_rank["ranking"], **t_it},
           "iterations": {"min": int(res.iterations.min()), "max": iters}, "largest_residual": float(res.residual.max()),
           "mutual_share_of_valid_edges": round(float((wr[valid] > 0).float().mean()), 4),
           "column_blocks": len(blocks), "row_bytes_of_a_gather": [4 * x for x in sorted(set(widths))],
           "gathered_bytes_per_iteration": gathered, "full_iteration_ms_all_blocks": round(it_ms, 4),
           "gather_bytes_over_full_iteration_time_TBps": round(gathered / (it_ms * 1e-3) / 1e12, 3) if it_ms > 0 else None,
           "graph_share_of_pipeline": round(t_graph["median_ms"] / (t_graph["median_ms"] + t_aff["median_ms"] + t_seeds["seeds"]["median_ms"]
                                                                    + t_solve["solve"]["median_ms"] + t_rank["ranking"]["median_ms"]), 3)}
    if "torch_cg" in t_solve:
        ref = out["torch_cg"]
        spread = max(t_solve[nm]["max_ms"] - t_solve[nm]["min_ms"] for nm in ("solve", "torch_cg"))
        rec["solve_over_torch_cg"] = round(t_solve["solve"]["median_ms"] / t_solve["torch_cg"]["median_ms"], 3)
        rec["largest_spread_ms"] = round(spread, 3)
        rec["difference_beyond_spread"] = bool(abs(t_solve["solve"]["median_ms"] - t_solve["torch_cg"]["median_ms"]) > spread)
        rec["max_column_difference_to_torch_cg_over_norm"] = float(((res.scores - ref).norm(dim=0) / ref.norm(dim=0).clamp_min(1e-30)).max())
    else:
        rec["torch_cg_error"] = torch_error
    return rec


def trace_run(dev):
    """one column block of 64 queries at n = 200000, d = 512, k = 50, 24 iterations in which no column stops: the subject of a kernel trace"""
    n, nq, d, k, kq = 200000, 64, 512, 50, 10
    v, _ = clustered_rows(1, n, d, 25, 0.6, dev)
    sc, ids = retrieval.knn_graph(v.t(), k)
    w = retrieval.mutual_knn_affinity(sc, ids, GAMMA)
    s, sid = retrieval.topk(v.t(), v[:nq].t(), kq)
    sw = s.clamp_min(0).pow(GAMMA)
    for _ in range(3):
        out = retrieval.diffuse(w, ids, sid, sw, ALPHA, 1e-30, 24)
    torch.cuda.synchronize()
    valid = int(((ids >= 0) & (ids < n)).sum())
    print(json.dumps({"iterations": [int(out.iterations.min()), int(out.iterations.max())], "gathered_bytes_per_spmv_launch": valid * 4 * nq}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="full", choices=sorted(SIZES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--graph-reps", type=int, default=2)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace", action="store_true", help="only the one-block run a kernel trace is taken of")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diffusion_bench measures on a GPU; none found")
    dev = torch.device("cuda:0")
    if a.trace:
        return trace_run(dev)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "tool": "tools/diffusion_bench.py", "reps": a.reps,
              "graph_reps": a.graph_reps, "shapes": []}
    cache = {}
    for n, nq, d, k, kq in SIZES[a.sizes]:
        rec = shape_record(n, nq, d, k, kq, a.reps, a.graph_reps, dev, cache)
        print(json.dumps(rec), flush=True)
        result["shapes"].append(rec)
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
