"""``CirDatasetAp`` (mdir/components/optim/score/cirscore.py:16-82): the mAP of a network on a cirtorch test dataset.

Descriptors, scores, ranks and the mAP stay on the device: the database and query images are decoded, cropped to the query bounding
boxes and resized by ``ImagesFromList`` (gandtr_amd/datasets.py), described by ``extract_vectors``, scored and ranked by
``scores_and_ranks`` and evaluated by the device ``compute_map_and_print`` (gandtr_amd/retrieval.py).  Two dataset forms, as the
reference: a name from cirtorch's ``DATASETS`` (``<data_root>/test/<name>/gnd_<name>.pkl``, images ``jpg/<name>.jpg``, data_root =
``$CIRTORCH_ROOT/data``) or a dict ``{"name", "queries", "db", "imgdir"}`` of TSV files (header row, tab separated, JSON cells for lists)."""
import gzip
import json
import lzma
import os
import pickle
import time

import torch

from .... import retrieval
from ....datasets import ImagesFromList
from ....ingest import DeviceTransform

DATASETS = ['oxford5k', 'paris6k', 'roxford5k', 'rparis6k', "247tokyo1k"]


def get_data_root():
    """cirtorch's data root: ``$CIRTORCH_ROOT/data`` (cirtorch/utils/general.py:4-11)"""
    root = os.environ.get("CIRTORCH_ROOT", "")
    if not root:
        raise ValueError("set CIRTORCH_ROOT: the cirtorch test datasets live in $CIRTORCH_ROOT/data/test/<name>")
    return os.path.join(root, "data")


def configdataset(dataset, dir_main):
    """image lists, query bounding boxes and ground truth of a named test dataset (cirtorch/datasets/testdataset.py:7-43)"""
    dataset = dataset.lower()
    if dataset not in DATASETS:
        raise ValueError('Unknown dataset: {}!'.format(dataset))
    gnd_fname = os.path.join(dir_main, dataset, 'gnd_{}.pkl'.format(dataset))
    with open(gnd_fname, 'rb') as f:
        cfg = pickle.load(f)
    images = os.path.join(dir_main, dataset, 'jpg')
    cfg.update(gnd_fname=gnd_fname, dataset=dataset, dir_data=os.path.join(dir_main, dataset), dir_images=images,
               n=len(cfg['imlist']), nq=len(cfg['qimlist']))
    cfg['images'] = [os.path.join(images, x + '.jpg') for x in cfg['imlist']]
    cfg['qimages'] = [os.path.join(images, x + '.jpg') for x in cfg['qimlist']]
    return cfg


def _cell(value):
    """a TSV cell: empty -> None, a JSON list / object -> its value, anything else the string"""
    if not value:
        return None
    if (value[0], value[-1]) in {("[", "]"), ("{", "}")}:
        return json.loads(value)
    return value


def read_table(path, keys):
    """columns ``keys`` of a .tsv / .csv file (optionally .gz / .xz), header row first: {key: [cell per row]}"""
    opener = gzip.open if path.endswith(".gz") else lzma.open if path.endswith(".xz") else open
    sep = "\t" if "tsv" in path.rsplit(".", 2) else ","
    with opener(path, "rb") as f:
        header = next(f).decode("utf8").strip().split(sep)
        cols = [header.index(k) for k in keys]
        out = {k: [] for k in keys}
        for line in f:
            cells = line.decode("utf8").strip("\n").split(sep)
            for k, c in zip(keys, cols):
                out[k].append(_cell(cells[c]))
    return out


def path_join(path, name, default_extension=".jpg"):
    """an image path from the image directory and an identifier (daan.ml.tools.path_join): absolute names stay; ``dir*ext`` gives the
    extension (``ext!`` replaces the name's own); a name with an extension keeps it; otherwise ``default_extension`` is appended"""
    if name.startswith("/"):
        return name
    ext = default_extension
    if "*" in path:
        path, ext = path.rsplit("*", 1)
    if "/" not in ext:
        if ext.endswith("!"):
            ext = ext[:-1]
            if ext:
                name = name.rsplit(".", 1)[0]
        elif "." in name.rsplit("/", 1)[-1] and name.rsplit(".", 1)[1]:
            ext = ""
    return os.path.join(path, name + ext)


class CirDatasetAp:

    decisive_criterion = "val/learning/score_avg:map_medium"

    def __init__(self, params):
        self.image_size = params.pop("image_size")
        self.dataset = params.pop("dataset")
        self.transforms = DeviceTransform(params.pop("transforms"), params.pop("mean_std"))
        if isinstance(self.dataset, dict):
            if self.dataset.keys() != {"name", "queries", "db", "imgdir"}:
                raise ValueError("a TSV dataset has the keys name, queries, db, imgdir; got %s" % sorted(self.dataset))
            imgdir = self.dataset["imgdir"]
            db = read_table(self.dataset["db"], ["identifier"])
            self.images = [path_join(imgdir, x) for x in db["identifier"]]
            index = {x: i for i, x in enumerate(db["identifier"])}
            qs = read_table(self.dataset["queries"], ["query", "bbx", "ok", "junk"])
            self.qimages = [path_join(imgdir, x) for x in qs["query"]]
            self.bbxs = [tuple(x) if x else None for x in qs["bbx"]]
            self.gnd = [{"ok": [index[x] for x in ok], "junk": [index[x] for x in junk]} for ok, junk in zip(qs["ok"], qs["junk"])]
            self.dataset = self.dataset["name"]
        else:
            cfg = configdataset(self.dataset, os.path.join(get_data_root(), "test"))
            self.images, self.qimages = cfg["images"], cfg["qimages"]
            self.bbxs = [tuple(cfg["gnd"][i]["bbx"]) if cfg["gnd"][i]["bbx"] else None for i in range(cfg["nq"])]
            self.gnd = cfg["gnd"]
        assert not params, params.keys()

    def _describe(self, network, device, images, bbxs=None, chunk=64):
        from ....stages.validate import extract_vectors
        data = ImagesFromList("", images, imsize=self.image_size, bbxs=bbxs, transform=self.transforms, device=device)
        cols = [extract_vectors(network, data.batch(range(lo, min(lo + chunk, len(data)))), device, batched=True)
                for lo in range(0, len(data), chunk)]
        return torch.cat(cols, dim=1)

    def __call__(self, network, device, logger):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("CirDatasetAp decodes, describes and ranks on a HIP device")
        t0 = time.time()
        print('>> {}: database images...'.format(self.dataset))
        vecs = self._describe(network, device, self.images)
        print('>> {}: query images...'.format(self.dataset))
        if self.images == self.qimages and set(self.bbxs) == {None}:
            qvecs = vecs.clone()
        else:
            qvecs = self._describe(network, device, self.qimages, self.bbxs)
        t1 = time.time()
        print('>> {}: Evaluating...'.format(self.dataset))
        _, ranks = retrieval.scores_and_ranks(vecs, qvecs)
        result = retrieval.compute_map_and_print(self.dataset, ranks, self.gnd)
        if result is None:
            raise ValueError("%s: the ground truth has no 'ok' lists and the dataset is not a revisited one (roxford5k*, rparis6k*)" % self.dataset)
        averages, scores = result
        t2 = time.time()
        first = scores[list(scores.keys())[0]]
        logger(None, len(first), "dataset", {"extract_descriptors": t1 - t0, "compute_score": t2 - t1}, "scalar/time")
        logger(None, len(first), "score_avg", averages, "scalar/score")
        assert len({len(x) for x in scores.values()}) == 1
        for i in range(len(first)):
            logger(i, len(first), "score", {x: scores[x][i] for x in scores}, "scalar/score")

    def __repr__(self):
        return "%s (dataset: %s, images: %d, queries: %d, image_size: %s)" % (type(self).__name__, self.dataset, len(self.images),
                                                                              len(self.qimages), self.image_size)
