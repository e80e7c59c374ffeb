"""dev tool: the GAN scenarios' training data on one device (gandtr_amd/components/data/dataset.py, gandtr_amd/csrc/crop_resize.hip).  64 pairs per batch
from JPEG files the tool writes itself with Pillow (1024 x 768, quality 90), through ``pil2np | scalecrop:256_256:0.8_1 | totensor | normalize``.
Timed per batch of 128 images, every variant warmed up first, the variants alternating inside this process:
  decode        jpeg.load_many of the batch's files (host parse + upload + device decode; host clock around a synchronise)
  plan          DeviceTransform.plan of the 64 items (host only)
  crop_resize   the gdt_crop_resize_u8_batch call alone on decoded tensors, writing into a preallocated batch (table build, one upload, one launch;
                device events over a burst)
  torch_ops     the same geometry with torch ops on the same tensors: slice -> permute -> float() / 255 -> F.interpolate(bilinear,
                align_corners=False) -> normalise -> stack
  loader_step   one whole batch of the loader (read + decode + plan + crop_resize; host clock around a synchronise)
Also: the largest difference between the two results (the coordinate maps agree at this power-of-two output size; torch rounds differently) and the
bytes the launch has to move against its time.  Event-timed bursts rank variants; they are not sustained-clock figures.
Prints one JSON line and writes it to the path given (default profiles/gan_data_1gpu.json).
usage: tools/gan_data_bench.py [iters] [out.json]      (default 10 timed samples per variant)"""
import json
import os
import random
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                               # noqa: E402
import torch                                                     # noqa: E402
import torch.nn.functional as F                                  # noqa: E402

from gandtr_amd import ingest, jpeg                              # noqa: E402
from gandtr_amd.components.data import dataset as D              # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 10
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gan_data_1gpu.json")
dev = torch.device("cuda:0")
PAIRS, FILES, H, W, BURST = 64, 48, 768, 1024, 20
MEAN_STD = [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]]


def write_files(root):
    from PIL import Image
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    for dom in "XY":
        names = []
        for i in range(FILES):
            rng = np.random.default_rng(100 * (dom == "Y") + i)
            a = np.stack([127 + 100 * np.sin(xx / (60 + i)) * np.cos(yy / 70), 127 + 90 * np.cos(xx / 50 + yy / (90 + i)), 60 + 0.1 * xx], -1)
            a = np.clip(a + rng.normal(0, 6, a.shape), 0, 255).astype(np.uint8)
            names.append("%s%02d.jpg" % (dom, i))
            Image.fromarray(a).save(os.path.join(root, names[-1]), quality=90)
        with open(os.path.join(root, dom + ".txt"), "w") as f:
            f.write("".join(n + "\n" for n in names))


def stats(v):
    v = sorted(v)
    return {"ms_median": round(v[len(v) // 2], 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4)}


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def burst_timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(BURST):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / BURST


def torch_ops(images, boxes):
    mean = torch.tensor(MEAN_STD[0], device=dev)[:, None, None]
    std = torch.tensor(MEAN_STD[1], device=dev)[:, None, None]
    out = []
    for img, (y0, x0, ch, cw) in zip(images, boxes):
        x = img[y0:y0 + ch, x0:x0 + cw].permute(2, 0, 1).float() / 255
        x = F.interpolate(x[None], size=(256, 256), mode="bilinear", align_corners=False)[0]
        out.append((x - mean) / std)
    return torch.stack(out)


with tempfile.TemporaryDirectory() as root, torch.no_grad():
    write_files(root)
    params = {"dataset": {"name": "RandomDomainsPair", "dataset_X": os.path.join(root, "X.txt"), "dataset_Y": os.path.join(root, "Y.txt"), "image_dir": root + "/*",
                          "size": PAIRS * 4},
              "loader": {"batch_size": PAIRS}, "transforms": "pil2np | scalecrop:256_256:0.8_1 | totensor | normalize", "mean_std": MEAN_STD}
    loader = D.initialize_dataset_loader(None, "train", params, device=dev)
    np.random.seed(0)
    random.seed(0)
    loader.dataset.prepare_epoch(None, None)
    ds, transform = loader.dataset, loader.dataset.transform
    batch0 = list(range(PAIRS))
    files = [f for i in batch0 for f in ds.files(i)]
    decoded = jpeg.load_many(files, dev)
    items = [decoded[2 * i:2 * i + 2] for i in range(PAIRS)]
    plans = [transform.plan([t.shape[:2] for t in item]) for item in items]
    boxes = [g.box for plan in plans for g in plan]
    out = torch.empty((len(decoded), 3, 256, 256), dtype=torch.float32, device=dev)

    variants = {
        "decode": (host_timed, lambda: jpeg.load_many(files, dev)),
        "plan": (host_timed, lambda: [transform.plan([t.shape[:2] for t in item]) for item in items]),
        "crop_resize": (burst_timed, lambda: ingest.crop_resize(decoded, boxes, 256, 256, None, MEAN_STD, out)),
        "torch_ops": (burst_timed, lambda: torch_ops(decoded, boxes)),
        "loader_step": (host_timed, lambda: loader.batch(batch0)),
    }
    for _, fn in variants.values():                               # warm-up of every variant
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(iters):
        for k, (timer, fn) in variants.items():
            times[k].append(timer(fn))
    got, ref = ingest.crop_resize(decoded, boxes, 256, 256, None, MEAN_STD), torch_ops(decoded, boxes)
    src_bytes = sum(ch * cw * 3 for _, _, ch, cw in boxes)
    out_bytes = got.numel() * 4
    # 16-byte table entries the call builds and uploads: a pic whose column / row geometry equals its predecessor's (the other pic of its pair) shares its table
    table_bytes = 16 * 256 * sum((i == 0 or (b[1], b[3]) != (boxes[i - 1][1], boxes[i - 1][3])) + (i == 0 or (b[0], b[2]) != (boxes[i - 1][0], boxes[i - 1][2]))
                                 for i, b in enumerate(boxes))
    rows = {k: stats(v) for k, v in times.items()}
    ms = rows["crop_resize"]["ms_median"]
    result = {"workload": "GAN training data: %d pairs per batch of %d x %d JPEG files (quality 90), scalecrop:256_256:0.8_1 -> 2 x %d x 3 x 256 x 256 fp32" % (PAIRS, W, H, PAIRS),
              "iters": iters, "burst": BURST, "images_per_batch": len(decoded), "per_batch": rows,
              "torch_ops_over_crop_resize": round(rows["torch_ops"]["ms_median"] / ms, 2),
              "max_abs_diff_to_torch_ops": float((got - ref).abs().max()),
              "crop_resize_bytes": {"source_boxes": src_bytes, "output": out_bytes, "tables_uploaded": table_bytes,
                                    "bytes_per_s": round((src_bytes + out_bytes + table_bytes) / (ms * 1e-3), 0)},
              "launches": {"crop_resize": 1, "torch_ops_per_image": "slice/permute views, float, div, interpolate, sub, div; one stack per batch"}}
line = json.dumps(result)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
