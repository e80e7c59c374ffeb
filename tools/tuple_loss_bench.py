"""Cost of the loss validation of the fine-tuning scenario on the device next to the reference's per-tuple loop, on the same GPU.

python tools/tuple_loss_bench.py [--json profiles/tuple_loss_1gpu.json] [--reps 20] [--tuples 1700] [--image-size 362] [--validation 1]
  kernel      gdt_tuple_loss alone (criterion.tuple_losses: the pair launch and the total launch) on 1700 tuples x 7 at d = 512 and d = 2048,
              clustered unit vectors, a random table on the device; device events around the call, the first call left out as warm-up, median of
              --reps.  Bytes: every pair reads its two rows (the anchor row once per tuple from memory, again from the cache), so the floor is
              T * S * d * 4 bytes at the 8.0 TB/s HBM peak; the record states the achieved rate over those bytes.
  validation  SingleValidation.validate (mining, every distinct image embedded once in batches, one loss launch) on a synthetic CirTuples set of
              --tuples pairs at --image-size (in-memory tensors, two aspect ratios, GeM-VGG16 with seeded weights), against the per-tuple loop of
              mdir/learning/validation.py:93-107 run through this repository's own path in the same process on the tuples just mined: seven
              batch-1 forwards (network.forward on the tuple's list), the criterion and one .item() per tuple.  Host wall time around each, the
              device synchronised before and after.  The mining is part of the first figure only (the reference mines as well, before its loop);
              it is reported separately so that the two loops can be compared alone."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gandtr_amd import mining                                               # noqa: E402
from gandtr_amd.components.optim import criterion as C                      # noqa: E402
from gandtr_amd.tools import synth, tensors                                 # noqa: E402

HBM_PEAK = 8.0e12


def clustered_unit_vectors(seed, d, n):
    rng = np.random.RandomState(seed)
    ncl = max(n // 10, 4)
    centres = rng.randn(d, ncl).astype(np.float32)
    v = centres[:, rng.randint(0, ncl, n)] + 0.7 * rng.randn(d, n).astype(np.float32)
    return (v / np.linalg.norm(v, axis=0, keepdims=True)).astype(np.float32)


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
    return out, float(np.median(ms[1:])), [round(x, 4) for x in ms[1:]]


def kernel_records(dev, tuples, s, reps):
    crit, records = C.ContrastiveLoss(0.75), []
    for d in (512, 2048):
        n_vec = tuples * 4
        vecs = torch.from_numpy(clustered_unit_vectors(0, d, n_vec)).to(dev)
        rows = vecs.t().contiguous().t()                                    # D x N view of [N][D] storage: the call adds no transpose pass
        table = torch.from_numpy(np.random.RandomState(1).randint(0, n_vec, (tuples, s)).astype(np.int32)).to(dev)
        out, ms, runs = timed(lambda: crit.tuple_losses(rows, table), reps)
        moved = tuples * s * d * 4
        records.append({"tuples": tuples, "s": s, "d": d, "kind": "contrastive", "call_ms": round(ms, 4), "call_ms_runs": runs, "launches": 2,
                        "row_bytes_read": moved, "achieved_TBps": round(moved / (ms * 1e-3) / 1e12, 3),
                        "hbm_floor_ms_at_8TBps": round(moved / HBM_PEAK * 1e3, 5), "times_the_hbm_floor": round(ms / (moved / HBM_PEAK * 1e3), 1),
                        "total": float(out.total)})
        print(json.dumps(records[-1]), flush=True)
    return records


def validation_record(dev, tuples, image_size, nnum=5):
    from gandtr_amd.learning import network as N
    from gandtr_amd.learning.validation import initialize_validation
    data = {"transforms": "pil2np | totensor | normalize", "mean_std": [[0.485, 0.456, 0.406], [0.229, 0.224, 0.225]]}
    emb = {"type": "SingleNetwork",
           "model": {"architecture": "cirnet", "cir_architecture": "vgg16", "local_whitening": False, "pooling": "gem", "pretrained": False,
                     "regional": False, "whitening": False},
           "initialize": False, "runtime": {"wrappers": "cirfaketuplebatch", "data": data}}
    net = N.initialize_network(emb, dev).eval()
    net.model.load_state_dict(synth.vgg16_state(0))
    nimg = 2 * tuples + tuples // 2
    short = int(round(image_size * 0.75))
    base = [synth.synth_input(k, (3, image_size, short) if k % 2 else (3, short, image_size)).to(dev) for k in range(16)]
    gen = torch.Generator(device=dev).manual_seed(0)
    images = [base[i % 16] + 0.25 * torch.randn(base[i % 16].shape, device=dev, generator=gen) for i in range(nimg)]
    db = {"qidxs": list(range(tuples)), "pidxs": [tuples + i for i in range(tuples)], "cluster": [i % tuples for i in range(nimg)]}
    crit = C.ContrastiveLoss(0.75)
    section = {"criterion": "default", "data": "val", "frequency": 5, "network_overlay": None, "type": "SingleValidation"}
    params = {"val": {"dataset": {"dataset": "synthetic", "dataset_pkl": None, "image_dir": "", "image_size": image_size, "name": "CirTuples",
                                  "neg_num": nnum, "pool_size": float("inf"), "query_size": float("inf"), "split": "val"},
                      "loader": {"batch_size": 1}}}
    val = initialize_validation(copy.deepcopy(section), data={"db": db, "images": images}, params_data=params, default_criterion=crit, network=net)
    times = {}
    torch.manual_seed(0)
    torch.cuda.synchronize()
    t0 = time.time()
    acc = val.validate(net, dev, lambda it, _n, label, value, _t: times.update(value) if label in ("prepare_epoch", "iteration") else None)
    torch.cuda.synchronize()
    whole = time.time() - t0
    ds = val.data_loader
    entries, table = mining.epoch_tuple_table(ds.qidxs, ds.pidxs, ds.nidxs, ds.tuple_labels)
    label = torch.tensor([-1., 1] + [0.] * nnum)
    torch.cuda.synchronize()
    t0 = time.time()
    loop = []
    with torch.no_grad():
        for t in range(tuples):
            batch = [tensors.as_metadata_tensor(images[i][None], {"image_label": [lab], "name": [str(i)]}) for i, lab in (entries[k] for k in table[t].tolist())]
            loop.append(crit(net.forward(batch), label).item())
    torch.cuda.synchronize()
    loop_s = time.time() - t0
    gap = float(np.abs(np.array(acc) - np.array(loop)).max())
    return {"tuples": tuples, "s": 2 + nnum, "image_size": image_size, "images": nimg, "distinct_entries_embedded": len(entries), "embedder": "GeM-VGG16",
            "validate_s": round(whole, 3), "of_which_mining_s": round(times.get("prepare_data", float("nan")), 3),
            "of_which_embed_and_loss_s": round(times.get("process_epoch", float("nan")), 3), "per_tuple_loop_s": round(loop_s, 3),
            "forwards_in_loop": tuples * (2 + nnum), "loop_over_embed_and_loss": round(loop_s / times["process_epoch"], 2),
            "mean_loss_batched": float(np.mean(acc)), "mean_loss_loop": float(np.mean(loop)), "max_abs_gap_per_tuple": gap}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tuples", type=int, default=1700)
    ap.add_argument("--image-size", type=int, default=362)
    ap.add_argument("--validation", type=int, default=1, help="0: the kernel alone")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tuple_loss_bench measures on a GPU; none found")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "tool": "tools/tuple_loss_bench.py",
           "kernel": kernel_records(dev, a.tuples, 7, a.reps)}
    if a.validation:
        out["validation"] = validation_record(dev, a.tuples, a.image_size)
        print(json.dumps(out["validation"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
