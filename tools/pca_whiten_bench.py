"""PCA whitening at descriptor size D on N vectors: pcawhitenlearn and pca_project_normalize on the GPU (whiten_learn.hip) next to the reference's
formulas in numpy on the host, and the covariance launch alone as the lower-tile form against the full tile grid.  Writes one JSON record.
usage: tools/pca_whiten_bench.py [--out profiles/pca_whiten_1gpu.json] [--sizes 2048x60000,512x20000] [--dims 128] [--no-cpu]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from gandtr_amd import _hip, whiten_learn


def median(values):
    return float(np.median(values))


def host_clock(fn, repeats):
    """seconds per call, host clock around a call that ends synchronised"""
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def covariance_ms(lib, rows, mean, c, lower, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.current_stream().cuda_stream
    start.record()
    for _ in range(repeats):
        _hip.check(lib.gdt_pca_covariance(rows.data_ptr(), rows.shape[0], rows.shape[1], mean.data_ptr(), c.data_ptr(), lower, stream))
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / repeats


def numpy_pcawhitenlearn(X):                     # cirtorch/utils/whiten.py:14-35, as written there
    N = X.shape[1]
    m = X.mean(axis=1, keepdims=True)
    Xc = X - m
    Xcov = np.dot(Xc, Xc.T)
    Xcov = (Xcov + Xcov.T) / (2 * N)
    eigval, eigvec = np.linalg.eig(Xcov)
    order = eigval.argsort()[::-1]
    eigval, eigvec = eigval[order], eigvec[:, order]
    return m, np.dot(np.linalg.inv(np.sqrt(np.diag(eigval))), eigvec.T)


def numpy_paste_pca_normalize(value, dimensions):       # mdir/stages/whiten.py:114-125, as written there
    value = value - np.mean(value)
    eigval, eigvec = np.linalg.eig(value.T.dot(value))
    vecs = eigvec[:, np.argsort(eigval)[-dimensions:]]
    value = value.dot(vecs.dot(vecs.T))
    return value / np.expand_dims(np.linalg.norm(value, axis=1), axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/pca_whiten_1gpu.json")
    ap.add_argument("--sizes", default="2048x60000,512x20000")
    ap.add_argument("--dims", type=int, default=128)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _hip.load()
    record = {"device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "dtype": "float64 (fp32 descriptor rows in)", "sizes": []}
    for size in args.sizes.split(","):
        d, n = (int(v) for v in size.split("x"))
        g = torch.Generator(device=dev).manual_seed(0)
        X = torch.nn.functional.normalize(torch.randn(n, d, generator=g, device=dev) * torch.linspace(1.5, 0.2, d, device=dev)[None, :], dim=1)   # N x D
        entry = {"d": d, "n": n, "covariance_gflop_full": round(2.0 * d * d * n / 1e9, 1)}
        # the covariance launch alone: full grid and lower tiles alternating, device events
        mean = X.double().mean(dim=0)
        c_full, c_low = torch.empty(d, d, dtype=torch.float64, device=dev), torch.empty(d, d, dtype=torch.float64, device=dev)
        reps = 3 if d >= 2048 else 10
        for lower, c in ((0, c_full), (1, c_low)):
            covariance_ms(lib, X, mean, c, lower, 1)                               # warm-up
        full, low = [], []
        for _ in range(5):
            full.append(covariance_ms(lib, X, mean, c_full, 0, reps))
            low.append(covariance_ms(lib, X, mean, c_low, 1, reps))
        entry["covariance_full_grid_ms"] = {"median": round(median(full), 3), "min": round(min(full), 3), "max": round(max(full), 3)}
        entry["covariance_lower_tiles_ms"] = {"median": round(median(low), 3), "min": round(min(low), 3), "max": round(max(low), 3)}
        entry["covariance_lower_over_full"] = round(median(low) / median(full), 3)
        entry["covariance_same_bits"] = bool(torch.equal(c_full, c_low))
        entry["covariance_lower_tflops_of_full_count"] = round(2.0 * d * d * n / (median(low) * 1e-3) / 1e12, 2)
        # the whole calls
        info = {}

        def learn():
            info["m"], info["P"], info["info"] = whiten_learn.pcawhitenlearn(X.t(), None, return_info=True)
        learn()
        t = host_clock(learn, 3)
        entry["pcawhitenlearn_s"] = {"median": round(median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
        entry["pcawhitenlearn_jacobi_sweeps"] = info["info"]["jacobi_sweeps"]
        entry["pcawhitenlearn_one_sided"] = info["info"]["one_sided"]
        Xc = X.double() - info["m"].t()
        C = Xc.t() @ Xc / n
        entry["max|P C P^T - I|"] = float((info["P"] @ C @ info["P"].t() - torch.eye(d, device=dev, dtype=torch.float64)).abs().max())
        del Xc, C
        V = X.double()

        def project():
            info["out"], info["pinfo"] = whiten_learn.pca_project_normalize(V, args.dims, return_info=True)
        project()
        t = host_clock(project, 3)
        entry["pca_project_normalize_dims"] = args.dims
        entry["pca_project_normalize_s"] = {"median": round(median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
        entry["pca_project_normalize_one_sided"] = info["pinfo"]["one_sided"]
        if not args.no_cpu:
            Xn = X.t().double().cpu().numpy()
            t0 = time.perf_counter()
            m_ref, P_ref = numpy_pcawhitenlearn(Xn)
            entry["numpy_pcawhitenlearn_s"] = round(time.perf_counter() - t0, 2)
            scale = 1.0 / np.linalg.norm(P_ref, axis=1, keepdims=True)
            P = info["P"].cpu().numpy()
            entry["unit_rows_up_to_sign_vs_numpy"] = float(np.minimum(np.linalg.norm((P - P_ref) * scale, axis=1),
                                                                      np.linalg.norm((P + P_ref) * scale, axis=1)).max())
            Vn = Xn.T.copy()
            del Xn
            t0 = time.perf_counter()
            ref = numpy_paste_pca_normalize(Vn, args.dims)
            entry["numpy_paste_pca_normalize_s"] = round(time.perf_counter() - t0, 2)
            entry["max|out - numpy|"] = float(np.abs(info["out"].cpu().numpy() - ref).max())
            del Vn, ref
        del V, info
        record["sizes"].append(entry)
        print(json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as handle:
        json.dump(record, handle, indent=1)
        handle.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
