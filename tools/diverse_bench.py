"""Cost of the diverse-anchor selection on the device next to the reference's loop as written, on the same GPU.

python tools/diverse_bench.py [--json profiles/diverse_anchors_1gpu.json] [--reps 5] [--baseline-reps 2] [--sizes scenario]
  Per size (qpool x qsize, descriptor size d) on clustered unit vectors, shuffle off:
    kernel path   retrieval.diverse_anchors (gdt_retrieval_diverse_anchors: 2 launches per step, no host round trip), device events around
                  the whole chain, the first call left out as warm-up, median of --reps;
    baseline      the loop of DiverseAnchorsDataset._select_positive_pairs_db (cirtorch_datasets.py:77-100) statement by statement in torch on
                  the same device -- torch.mm, torch.cat onto the growing matrix, max(dim=1), a full argsort, two .item() -- one warm-up
                  run, median of --baseline-reps.  The kernel path is never compared with itself.
  The record also states how far the chain is from streaming the descriptor matrix once per step (steps * qpool * d * 4 bytes) at the
  8.0 TB/s HBM peak, and how many picks of the two paths coincide (they may part where neighbours are closer than fp32 rounding).
  The split between the two kernels comes from one run under ``rocprofv3 --kernel-trace --stats``, in a run of its own."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gandtr_amd import retrieval                                            # noqa: E402

HBM_PEAK = 8.0e12
SIZES = {"scenario": [(10000, 2000, 512), (10000, 2000, 2048), (1000, 200, 128)], "small": [(1000, 200, 128)]}


def clustered_unit_vectors(seed, d, n):
    rng = np.random.RandomState(seed)
    ncl = max(n // 10, 4)
    centres = rng.randn(d, ncl).astype(np.float32)
    v = centres[:, rng.randint(0, ncl, n)] + 0.7 * rng.randn(d, n).astype(np.float32)
    return (v / np.linalg.norm(v, axis=0, keepdims=True)).astype(np.float32)


def reference_loop(qvecs, qsize, similar_exclude, similar_include):
    """cirtorch_datasets.py:77-100 with shuffle off"""
    qpool_size = qvecs.shape[1]
    with torch.no_grad():
        idx = 0
        idxs = [idx]
        dists = torch.empty(qpool_size, 0, device=qvecs.device)
        qscore_acc = []
        for _ in range(qsize - 1):
            dist = torch.mm(qvecs.t(), qvecs[:, idx:idx + 1])
            dists = torch.cat([dists, dist], dim=1)
            most_similar = dists.max(dim=1)[0]
            valid_size = qpool_size - len(idxs)
            similar_split = max(int(valid_size * (1 - similar_exclude)), 1)
            dissimilar_split = min(int(valid_size * (1 - similar_include)), similar_split - 1)
            dissimilar_part = most_similar.argsort()[dissimilar_split:similar_split]
            choice = dissimilar_part.shape[0] - 1
            idx = dissimilar_part[choice].item()
            qscore_acc.append(most_similar[idx].item())
            idxs.append(idx)
    return idxs, qscore_acc


def timed(fn, reps):
    ms, out = [], None
    for _ in range(reps + 1):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return out, float(np.median(ms[1:])), [round(x, 3) for x in ms[1:]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="scenario", choices=sorted(SIZES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-reps", type=int, default=2)
    ap.add_argument("--baseline", type=int, default=1, help="0: kernel path only (for a profiler run)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diverse_bench measures on a GPU; none found")
    dev = torch.device("cuda:0")
    exclude, include = 0.2, 0.8
    records = []
    for qpool, qsize, d in SIZES[a.sizes]:
        qvecs = torch.from_numpy(clustered_unit_vectors(0, d, qpool)).to(dev)
        targets = retrieval.diverse_anchor_targets(qpool, qsize, exclude, include, False)
        (idxs, scores), k_ms, k_all = timed(lambda: retrieval.diverse_anchors(qvecs, targets), a.reps)
        steps = qsize - 1
        moved = steps * qpool * d * 4
        rec = {"qpool": qpool, "qsize": qsize, "d": d, "similar_exclude": exclude, "similar_include": include, "shuffle": False,
               "kernel_chain_ms": round(k_ms, 3), "kernel_chain_ms_runs": k_all, "launches": 2 * steps,
               "per_step_us": round(k_ms * 1e3 / steps, 3), "matrix_bytes_streamed": moved,
               "achieved_TBps": round(moved / (k_ms * 1e-3) / 1e12, 3), "stream_floor_ms_at_8TBps": round(moved / HBM_PEAK * 1e3, 3),
               "times_the_stream_floor": round(k_ms / (moved / HBM_PEAK * 1e3), 2)}
        if a.baseline:
            (ref_idxs, ref_scores), t_ms, t_all = timed(lambda: reference_loop(qvecs, qsize, exclude, include), a.baseline_reps)
            got = idxs.cpu().tolist()
            same = sum(int(x == y) for x, y in zip(got, ref_idxs))
            first_diff = next((i for i, (x, y) in enumerate(zip(got, ref_idxs)) if x != y), None)
            rec.update({"torch_reference_loop_ms": round(t_ms, 1), "torch_reference_loop_ms_runs": t_all,
                        "speedup_over_torch_loop": round(t_ms / k_ms, 1), "picks_equal_to_torch_loop": same,
                        "first_differing_step": first_diff,
                        "mean_score_kernel": round(float(scores.mean()), 6), "mean_score_torch_loop": round(float(np.mean(ref_scores)), 6)})
        print(json.dumps(rec), flush=True)
        records.append(rec)
    if a.json:
        out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "tool": "tools/diverse_bench.py", "records": records}
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
