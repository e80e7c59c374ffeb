"""Generate tests/golden/gan_data.npz by IMPORTING THE REFERENCE's transforms and datasets (read-only) -- the way make_gan_objective_golden.py does.

Runs only where the reference is present.  The cases live in tests/gan_data_fixture.py; the file holds recorded results only (boxes, flags, drawn
numbers, picked indices, Pillow's downscaled pixels).

Crop geometry: ``cv2`` is a placeholder here, so ``cv2.resize`` is replaced by a recorder.  The pics are coordinate images (channel 0 = y * W + x,
channel 1 = W): the slice the reference hands to ``cv2.resize`` -- or returns, for the plain crops -- tells its source box and whether it was mirrored
before; the recorder's result is a column ramp, so a mirror after the resize shows too.  Per case and seed: ``<case>_box`` [seeds][pics][4] = (y0, x0,
ch, cw) in the unmirrored pic, ``_flip_src`` / ``_flip_dst`` / ``_resampled`` [seeds][pics], ``_next`` [seeds] = ``random.random()`` right after the call,
``_refused`` [seeds] = 1 where the reference's own assert fired (everything else of that row is then -1).

usage:  python tests/golden/make_gan_data_golden.py
"""
import os
import pickle
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden                                             # noqa: E402  (placeholders, paths)
import gan_data_fixture as FX                                  # noqa: E402

RESIZED = -7.0                                                 # channel 1 of what the recorder returns


def box_of(view):
    """(y0, x0, ch, cw, mirrored) of a slice (possibly mirrored) of a coordinate pic"""
    w = int(view[0, 0, 1])
    first, last = int(view[0, 0, 0]), int(view[0, -1, 0])
    y0, xa, xb = first // w, first % w, last % w
    return y0, min(xa, xb), view.shape[0], abs(xa - xb) + 1, int(xb < xa)


def main():
    make_golden._install_placeholders()
    sys.path.insert(0, make_golden.REF)
    import torch
    threads = torch.get_num_threads()
    import mdir                                                     # noqa: F401
    torch.set_num_threads(threads)
    import cv2
    from mdir.components.data import transform as ref_transform
    from mdir.components.data.dataset import domain_datasets, tuple_datasets

    seen = []

    def resize(src, dsize, *args, **kwargs):
        seen.append(box_of(src))
        out = np.zeros((dsize[1], dsize[0], 3), dtype=np.float32)
        out[..., 0] = np.arange(dsize[0], dtype=np.float32)[None, :]
        out[..., 1] = RESIZED
        out[..., 2] = len(seen) - 1
        return out
    cv2.resize = resize

    arrays = {}
    for name, (chain, shapes) in FX.CROP_CASES.items():
        compose = ref_transform.initialize_transforms(chain, None)
        rows = {k: [] for k in ("box", "flip_src", "flip_dst", "resampled", "next", "refused")}
        for seed in FX.SEEDS:
            pics = [FX.coordinate_pic(h, w) for h, w in shapes]
            del seen[:]
            random.seed(seed)
            try:
                out = compose(*pics)
            except AssertionError:
                for k in ("box", "flip_src", "flip_dst", "resampled"):
                    rows[k].append(np.full((len(shapes), 4) if k == "box" else len(shapes), -1))
                rows["next"].append(-1.0)
                rows["refused"].append(1)
                continue
            rows["next"].append(random.random())
            rows["refused"].append(0)
            out = [out] if len(shapes) == 1 else list(out)
            box, fs, fd, rs = [], [], [], []
            for res in out:
                if res[0, 0, 1] == RESIZED:
                    y0, x0, ch, cw, mirrored = seen[int(res[0, 0, 2])]
                    fd.append(int(res[0, 0, 0] != 0))
                    rs.append(1)
                else:
                    y0, x0, ch, cw, mirrored = box_of(res)
                    fd.append(0)
                    rs.append(0)
                box.append((y0, x0, ch, cw))
                fs.append(mirrored)
            for k, v in zip(("box", "flip_src", "flip_dst", "resampled"), (box, fs, fd, rs)):
                rows[k].append(np.asarray(v))
        for k, v in rows.items():
            arrays["%s_%s" % (name, k)] = np.asarray(v, dtype=np.float64 if k == "next" else np.int64)

    for name, ((h, w), n) in FX.DOWNSCALE_CASES.items():
        pic = FX.photo(11, h, w).astype(np.float32) / 255.0
        out = ref_transform.initialize_transforms("downscale:%d" % n, None)(pic)
        arrays[name] = np.asarray(out, dtype=np.float32)

    with tempfile.TemporaryDirectory() as tmp:
        for name, (nx, ny, size, seed) in FX.PAIR_CASES.items():
            for dom, count in (("X", nx), ("Y", ny)):
                with open(os.path.join(tmp, "%s_%s.txt" % (name, dom)), "w") as f:
                    f.write("".join("%s%d.jpg\n" % (dom, i) for i in range(count)))
            ds = domain_datasets.RandomDomainsPairDataset(None, None, os.path.join(tmp, name + "_X.txt"), os.path.join(tmp, name + "_Y.txt"), tmp + "/*", size)
            np.random.seed(seed)
            ds.prepare_epoch(None, None)
            arrays[name + "_X"], arrays[name + "_Y"] = np.asarray(ds.idxs_X, dtype=np.int64), np.asarray(ds.idxs_Y, dtype=np.int64)
            arrays[name + "_len"] = np.asarray(len(ds))
        names = FX.tuple_names()
        with open(os.path.join(tmp, "tuples.pkl"), "wb") as f:
            pickle.dump({"val": names, "other": []}, f)
        for idx in FX.TUPLE_IDX:
            ds = tuple_datasets.PregeneratedImageTupleDataset(None, None, os.path.join(tmp, "tuples.pkl"), "val", tmp + "/*", idx)
            picks = [[possible.index(os.path.basename(p)) for p in chosen] for possible, chosen in zip(names, ds.epoch_images)]
            arrays["tuple_" + idx] = np.asarray(picks, dtype=np.int64)

    path = os.path.join(HERE, "gan_data.npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s: %d arrays, %.1f KiB" % (path, len(arrays), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
