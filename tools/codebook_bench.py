"""dev tool: the codebook kernels and the local head against the reference's op sequence in torch ops on the same GPU, in one process, alternating
after a warm-up; medians of 5 with min..max.  Writes profiles/codebook_1gpu.json (or the path given).

Rows (the baseline of every row is torch, never the code under test):
  nearest      F = 131072 features (32 maps of 64 x 64), K = 65536 centroids, D = 128 / 512, ma = 1 / 3: gdt_codebook_nearest against cdist + topk in blocks
               of 1,000,000 distances, as Codebook._chunk_weights_topk walks them.  TFLOP/s = 2 F K D / time, against the 157 TF fp32 matrix peak.
  aggregate    the same sizes, normresatt / l2norm: gdt_codebook_aggregate against an index_add_ restatement -- the reference's dense
               centroids x dim x features scratch (grouping.py:120-124) cannot exist at these sizes (137 GB per image at D = 128), so the baseline is NOT the
               reference's op sequence here.
  kmeans       one iteration at 10^6 x 128 points and 65536 clusters: nearest + gdt_kmeans_update against blocked cdist + argmin (blocks of 2^28 distances; the
               reference's single cdist would be 262 GB) and an index_add_ mean (its one-masked-mean-per-centroid loop is 65536 launches over 10^6 points).
  local_head   32 x 64 x 64 x 512 and 32 x 32 x 32 x 2048 fp16 maps: gdt_local_descriptors against permute + norm + divide (and the attention) in torch.
               TB/s = (map in + descriptors and attention out) / time.
usage: tools/codebook_bench.py [output.json] [--quick]"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch                                                     # noqa: E402

from gandtr_amd import codebook, engine                          # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
quick = "--quick" in sys.argv
path = args[0] if args else os.path.join("profiles", "codebook_1gpu.json")
dev = torch.device("cuda:0")
REPS = 5
PEAK_TF = 157.0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    v = sorted(v)
    return {"ms_median": round(v[len(v) // 2], 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4)}


def alternate(fns, n=REPS):
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(n):                                            # alternating: all see the same clocks / neighbours
        for k, fn in fns.items():
            t[k].append(timed(fn))
    return {k: stats(v) for k, v in t.items()}


def data(F, K, D, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    c = torch.randn(K, D, device=dev, generator=g)
    x = c[torch.randint(0, K, (F,), device=dev, generator=g)] + 0.7 * torch.randn(F, D, device=dev, generator=g)
    return x, c


def torch_nearest(x, c, ma, block=1_000_000):
    step = max(block // c.shape[0], 1)
    ds, ids = [], []
    for s in range(0, x.shape[0], step):
        d, i = torch.topk(torch.cdist(x[s:s + step], c), ma, dim=1, largest=False, sorted=True)
        ds.append(d)
        ids.append(i)
    return torch.cat(ds), torch.cat(ids)


def torch_aggregate(x, att, c, ids, ass, n_images, per_image):
    K, D = c.shape
    r = x.unsqueeze(1) - c[ids.long()]
    feat = att.view(-1, 1, 1) * (r / (torch.norm(r, dim=-1, keepdim=True) + 1e-6))
    key = (torch.arange(x.shape[0], device=x.device) // per_image).unsqueeze(1) * K + ids.long()
    dense = torch.zeros(n_images * K, D, device=x.device)
    dense.index_add_(0, key.reshape(-1), (feat * ass.unsqueeze(2)).reshape(-1, D))
    return (dense / (torch.norm(dense, dim=1, keepdim=True) + 1e-6)).view(n_images, K, D)


def torch_kmeans_step(x, c, block=1 << 28):
    step = max(block // c.shape[0], 1)
    ids = torch.cat([torch.cdist(x[s:s + step], c).argmin(dim=1) for s in range(0, x.shape[0], step)])
    sums = torch.zeros_like(c).index_add_(0, ids, x)
    cnt = torch.zeros(c.shape[0], device=x.device).index_add_(0, ids, torch.ones(x.shape[0], device=x.device))
    return torch.where(cnt.unsqueeze(1) > 0, sums / cnt.clamp(min=1).unsqueeze(1), c)


def torch_local(nchw_view):
    ss = nchw_view.float().pow(2).sum(1, keepdim=True)
    return (nchw_view.float() / (ss.sqrt() + 1e-6)).contiguous(), (ss.squeeze(1) + 1e-10).sqrt()


out = {"workload": "codebooks: nearest / aggregate / k-means / local head against torch ops on the same GPU, one process, alternating", "reps": REPS, "rows": {}}
F, K, I = (8192, 4096, 8) if quick else (131072, 65536, 32)
for D in (128, 512):
    x, c = data(F, K, D, D)
    att = torch.rand(F, device=dev) + 0.1
    for ma in (1, 3):
        row = alternate({"kernel": lambda: codebook.nearest(x, c, ma), "torch_cdist_topk_blocks_of_1e6": lambda: torch_nearest(x, c, ma)})
        (dk, ik), (dt, it) = codebook.nearest(x, c, ma), torch_nearest(x, c, ma)
        row["ids_equal_to_torch"] = float((ik.long() == it).float().mean())
        row["max_abs_dist_diff"] = float((dk - dt).abs().max())
        row["kernel_tflops"] = round(2.0 * F * K * D / (row["kernel"]["ms_median"] * 1e-3) / 1e12, 2)
        row["kernel_share_of_fp32_matrix_peak"] = round(row["kernel_tflops"] / PEAK_TF, 3)
        row["speedup_over_torch"] = round(row["torch_cdist_topk_blocks_of_1e6"]["ms_median"] / row["kernel"]["ms_median"], 2)
        out["rows"]["nearest F=%d K=%d D=%d ma=%d" % (F, K, D, ma)] = row
        ass = torch.softmax(-2.0 * dk, dim=1)
        sizes = [F // I] * I
        row = alternate({"kernel": lambda: codebook.aggregate(x, att, c, ik, ass, sizes, "normresatt", "l2norm"),
                         "torch_index_add_restatement": lambda: torch_aggregate(x, att, c, ik, ass, I, F // I)})
        g = codebook.aggregate(x, att, c, ik, ass, sizes, "normresatt", "l2norm")[0]
        row["max_abs_diff_to_torch"] = float((g - torch_aggregate(x, att, c, ik, ass, I, F // I)).abs().max())
        row["output_gb"] = round(I * K * D * 4 / 1e9, 3)
        row["kernel_output_tb_per_s"] = round(I * K * D * 4 / (row["kernel"]["ms_median"] * 1e-3) / 1e12, 3)
        row["speedup_over_torch"] = round(row["torch_index_add_restatement"]["ms_median"] / row["kernel"]["ms_median"], 2)
        row["baseline_note"] = "index_add_ restatement: the reference's dense centroids x dim x features scratch cannot exist at this size"
        out["rows"]["aggregate I=%d F=%d K=%d D=%d ma=%d normresatt/l2norm" % (I, F, K, D, ma)] = row
        del g, ass
    del x, c
    torch.cuda.empty_cache()

P, KC = (65536, 4096) if quick else (1_000_000, 65536)
x, c = data(P, KC, 128, 7)


def kernel_step():
    work = c.clone()
    codebook.kmeans_update(x, codebook.nearest(x, work, 1)[1], work)
    return work


row = alternate({"kernel_nearest_plus_update": kernel_step, "torch_blocked_cdist_argmin_index_add": lambda: torch_kmeans_step(x, c)})
row["max_abs_diff_to_torch"] = float((kernel_step() - torch_kmeans_step(x, c)).abs().max())
row["kernel_tflops"] = round(2.0 * P * KC * 128 / (row["kernel_nearest_plus_update"]["ms_median"] * 1e-3) / 1e12, 2)
row["speedup_over_torch"] = round(row["torch_blocked_cdist_argmin_index_add"]["ms_median"] / row["kernel_nearest_plus_update"]["ms_median"], 2)
row["baseline_note"] = "blocks of 2^28 distances and an index_add_ mean, not the reference's one masked mean per centroid"
out["rows"]["kmeans one iteration points=%d clusters=%d D=128" % (P, KC)] = row
del x, c
torch.cuda.empty_cache()

for n, h, w, d in ((4, 16, 16, 512),) if quick else ((32, 64, 64, 512), (32, 32, 32, 2048)):
    nhwc = torch.relu(torch.randn(n, h, w, d, device=dev)).half()
    view = nhwc.permute(0, 3, 1, 2)                               # the same memory under torch's NCHW indexing
    row = alternate({"kernel": lambda: engine.local_descriptors(nhwc), "torch_permute_norm": lambda: torch_local(view)})
    (dk, ak), (dt, at) = engine.local_descriptors(nhwc), torch_local(view)
    row["max_abs_diff_to_torch"] = float(max((dk - dt).abs().max(), ((ak - at).abs() / at.abs().clamp(min=1e-6)).max()))
    nbytes = n * h * w * d * 2 + n * h * w * d * 4 + n * h * w * 4
    row["kernel_tb_per_s"] = round(nbytes / (row["kernel"]["ms_median"] * 1e-3) / 1e12, 3)
    row["speedup_over_torch"] = round(row["torch_permute_norm"]["ms_median"] / row["kernel"]["ms_median"], 2)
    out["rows"]["local_head %d x %d x %d x %d f16" % (n, h, w, d)] = row
    del nhwc, view
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
with open(path, "w") as handle:
    json.dump(out, handle, indent=1)
    handle.write("\n")
print(json.dumps(out))
