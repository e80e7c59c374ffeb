"""Datasets and loaders of the GAN scenarios' ``data:`` blocks: this repository's counterpart of the reference's ``mdir.components.data.dataset``
(``DATASET_LABELS``, ``initialize_dataset``, ``initialize_dataset_loader``; its tuple and domain datasets).  Written from the behaviour that
tests/golden/gan_data.npz pins -- which random source is asked for what, in which order; how an index rule picks a file of a tuple; how a directory
pattern and a name make a path -- not from the reference's text.

The reference gives a ``torch.utils.data.Dataset`` whose ``__getitem__`` decodes with Pillow and transforms on the CPU to a ``DataLoader`` with worker
processes.  Here a dataset is a table of file paths (``files(i)``: the paths of item i, one per column) and the loader, ``BatchLoader``, does the work
of a whole batch at once on the device: ONE ``jpeg.load_many`` for all files of all columns, one ``DeviceTransform.plan`` per item (host; items in
index order, so the random draws are those of a single-process reference run), ONE ``DeviceTransform.apply_many``.  It yields what the reference's
loader collates: one fp32 N x 3 x h x w device tensor per column -- a list of them, or the tensor itself for a one-column dataset, because the
reference's ``Compose`` hands back a single pic unwrapped -- and ``[names, images]`` for ``InferImageList``.  With a CPU ``device`` the same classes run
through the host transforms and Pillow (``__getitem__`` + ``default_collate``): plumbing for hosts without a GPU.  The HIP route has no CPU fallback.

Not provided: the ``Cir*`` datasets (gandtr_amd.mining / gandtr_amd.learning.validation have them), HDF5 tuple files, the reference's path rewriting
rules (paths are taken as given, environment variables expanded), worker processes."""
import math
import os
import pickle
import random

import numpy as np
import torch

from .transform import initialize_transforms


def image_path(directory, name):
    """Path of image ``name`` under a directory pattern.  An absolute name wins.  The pattern is ``dir`` (names without an extension get ``.jpg``) or
    ``dir/*suffix``: a suffix that is a plain extension is added only to names that have none, ``ext!`` replaces whatever extension the name has, and a
    suffix that continues the path (contains ``/``) is appended as it is."""
    if name.startswith("/"):
        return name
    prefix, star, suffix = directory.rpartition("*")
    if not star:
        prefix, suffix = directory, ".jpg"
    if "/" not in suffix:
        leaf = name.rsplit("/", 1)[-1]
        if suffix.endswith("!"):
            suffix = suffix[:-1]
            if suffix and "." in name:
                name = name[:name.rindex(".")]
        elif "." in leaf and not leaf.endswith("."):
            suffix = ""
    return os.path.join(prefix, name + suffix)


def _expand(path):
    return os.path.expandvars(path) if isinstance(path, str) else path


def read_tuples(path, key):
    """column ``key`` of a tuple file: a pickled dict of lists"""
    kind = path.rsplit(".", 1)[-1].lower()
    if kind in ("h5", "hdf5"):
        raise NotImplementedError("HDF5 tuple files are not supported ('%s')" % path)
    if kind != "pkl":
        raise ValueError("Suffix '%s' is not supported ('%s')" % (kind, path))
    with open(path, "rb") as handle:
        return pickle.load(handle)[key]


def _read_names(path):
    with open(_expand(path)) as handle:
        return [line.strip() for line in handle]


def _open_image(path, mode):
    from PIL import Image
    with open(path, "rb") as handle:
        return Image.open(handle).convert(mode or "RGB")


class FileDataset:
    """A table of image files: ``files(i)`` are the paths of item i, one per column, ``names(i)`` what is yielded beside the images (or None).
    ``__getitem__`` is the host route: Pillow, then ``transform(*pics)``."""

    loader_params = {}
    mode = None
    transform = None

    def files(self, index):
        raise NotImplementedError

    def names(self, index):
        return None

    def prepare_epoch(self, network, device):
        return None

    def __getitem__(self, index):
        pics = tuple(_open_image(path, self.mode) for path in self.files(index))
        if self.transform:
            pics = self.transform(*pics)
        label = self.names(index)
        return pics if label is None else (label, pics)


class ImageListDataset(FileDataset):
    """``data``: equally long columns of names; item i is row i across the columns"""

    def __init__(self, data, transform, image_dir, mode=None):
        lengths = {len(column) for column in data}
        assert len(lengths) == 1, "columns of different lengths: %s" % sorted(lengths)
        directory = _expand(image_dir)
        self.rows = [list(row) for row in zip(*data)]
        self.paths = [[image_path(directory, name) for name in row] for row in self.rows]
        self.transform, self.mode = transform, mode

    def __len__(self):
        return len(self.paths)

    def files(self, index):
        return self.paths[index]


class InferImageListDataset(ImageListDataset):
    """... and the names travel with the images: items are ``(names, images)``"""

    def names(self, index):
        return tuple(self.rows[index])


def pick_index(rule, count, taken, rand):
    """Which of a tuple's ``count`` files a column shows.  ``rule``: an int (negative counts from the end), ``"any"`` = ``rand(count)``,
    ``"different"`` = one of the positions not in ``taken``, chosen by ``rand(how many are left)``, or a pair of bounds = ``rand(low or 0, high or
    count)``; the bounds must lie inside the tuple (negative ones after wrapping) but reach ``rand`` as they were given."""
    def inside(i):
        wrapped = i + count if i < 0 else i
        assert 0 <= wrapped < count, "index %d outside a tuple of %d" % (i, count)
        return wrapped

    if rule == "any":
        return rand(count)
    if rule == "different":
        free = [i for i in range(count) if i not in taken]
        return free[rand(len(free))]
    if isinstance(rule, (list, tuple)):
        for bound in rule:
            if bound is not None:
                inside(bound)
        low, high = rule
        return rand(low or 0, high or count)
    return inside(rule)


class RandomImageTupleDataset(FileDataset):
    """Tuples of files (a pickled list under ``data_key``); each column shows the file its rule in ``idx`` picks (``"0_any"``: column 0 the first file,
    column 1 any).  ``prepare_epoch`` picks anew with ``np.random.randint``, tuple by tuple, column by column."""

    def __init__(self, data, transform, dataset, data_key, image_dir, idx):
        assert not data, "a tuple dataset reads its own file"
        directory = _expand(image_dir)
        self.tuples = [[image_path(directory, name) for name in names] for names in read_tuples(_expand(dataset), data_key)]
        self.transform = transform
        self.idx = [part if part in ("any", "different") else int(part) for part in idx.split("_")] if isinstance(idx, str) else idx
        self.epoch_idxs = self.epoch_images = None

    get_idx = staticmethod(pick_index)

    def draw(self, rand):
        self.epoch_idxs = []
        for files in self.tuples:
            picked = []
            for rule in self.idx:
                picked.append(int(pick_index(rule, len(files), picked, rand)))
            self.epoch_idxs.append(picked)
        self.epoch_images = [[files[i] for i in picked] for files, picked in zip(self.tuples, self.epoch_idxs)]

    def prepare_epoch(self, network, device):
        self.draw(np.random.randint)

    def __len__(self):
        return len(self.tuples)

    def files(self, index):
        return self.epoch_images[index]


class PregeneratedImageTupleDataset(RandomImageTupleDataset):
    """... picked ONCE, at construction, from ``random.Random(0).randrange``: every run (and a run resumed from a checkpoint) sees the same tuples"""

    def __init__(self, data, transform, dataset, data_key, image_dir, idx):
        super().__init__(data, transform, dataset, data_key, image_dir, idx)
        self.draw(random.Random(0).randrange)

    def prepare_epoch(self, network, device):
        return None


class RandomDomainsPairDataset(FileDataset):
    """Unpaired images of two domains (two name lists): item i is (X[a_i], Y[b_i]) with a and b drawn per epoch, with replacement --
    ``np.random.randint(len(X), size=size)`` first, then the same for Y.  ``size`` None: the shorter list's length."""

    def __init__(self, data, transform, dataset_X, dataset_Y, image_dir, size, image_dir_Y=None):
        assert not data, "a domain-pair dataset reads its own lists"
        dir_x = _expand(image_dir)
        dir_y = dir_x if image_dir_Y is None else _expand(image_dir_Y)
        self.images_X = [image_path(dir_x, name) for name in _read_names(dataset_X)]
        self.images_Y = [image_path(dir_y, name) for name in _read_names(dataset_Y)]
        self.transform = transform
        self.size = min(len(self.images_X), len(self.images_Y)) if size is None else int(size)
        self.idxs_X = self.idxs_Y = None

    def prepare_epoch(self, network, device):
        self.idxs_X = np.random.randint(len(self.images_X), size=self.size).tolist()
        self.idxs_Y = np.random.randint(len(self.images_Y), size=self.size).tolist()

    def __len__(self):
        return self.size

    def files(self, index):
        return [self.images_X[self.idxs_X[index]], self.images_Y[self.idxs_Y[index]]]


DATASET_LABELS = {
    "ImageList": ImageListDataset,
    "InferImageList": InferImageListDataset,
    "RandomImageTuple": RandomImageTupleDataset,
    "PregeneratedImageTuple": PregeneratedImageTupleDataset,
    "RandomDomainsPair": RandomDomainsPairDataset,
}
_ELSEWHERE = ("CirTuples", "CirDiverseAnchors", "CirImageList")

LOADER_DEFAULT_PARAMS = dict(shuffle=False, num_workers=6, pin_memory=True)


class BatchLoader:
    """An iterable over whole batches of a ``FileDataset`` (module docstring).  ``shuffle`` draws ``torch.randperm`` on the host; ``num_workers`` /
    ``pin_memory`` are accepted and ignored; ``loader`` is the caller's ``bytes -> H x W x 3 uint8 array`` function for files the device decoder
    refuses (PNG, CMYK JPEG ...), as in ``ImagesFromList``."""

    def __init__(self, dataset, batch_size, shuffle=False, num_workers=0, pin_memory=False, drop_last=False, device=None, loader=None):
        self.dataset, self.batch_size, self.shuffle, self.drop_last, self.loader = dataset, int(batch_size), bool(shuffle), bool(drop_last), loader
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.batch_size < 1:
            raise ValueError("batch_size should be a positive integer value, but got batch_size=%s" % batch_size)

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else math.ceil(n / self.batch_size)

    def __iter__(self):
        n = len(self.dataset)
        order = torch.randperm(n).tolist() if self.shuffle else list(range(n))
        for k in range(len(self)):
            yield self.batch(order[k * self.batch_size:(k + 1) * self.batch_size])

    def batch(self, indices):
        indices = list(indices)
        if self.device.type == "cpu":
            from torch.utils.data import default_collate
            return default_collate([self.dataset[i] for i in indices])
        from ... import jpeg
        ds = self.dataset
        if ds.mode not in (None, "RGB"):
            raise NotImplementedError("image mode '%s' is not supported on the HIP path" % ds.mode)
        files = [ds.files(i) for i in indices]
        decoded = iter(jpeg.load_many([f for item in files for f in item], self.device, host_loader=self.loader))
        items = [[next(decoded) for _ in item] for item in files]
        plans = [ds.transform.plan([t.shape[:2] for t in item]) for item in items]
        columns = ds.transform.apply_many(items, plans)
        images = columns[0] if len(columns) == 1 else columns
        names = [ds.names(i) for i in indices]
        return images if names[0] is None else [[tuple(col) for col in zip(*names)], images]


def initialize_dataset(data, stage, transform, params):
    """``params``: ``name`` (a key of ``DATASET_LABELS``) and the dataset's own arguments.  In the train and val stages ``data_cols`` = ``"first:last"``
    (``last`` may be empty) selects the columns of ``data`` the dataset sees; the test stage takes ``data`` whole."""
    if stage not in ("train", "val", "test"):
        raise RuntimeError("Unsupported stage '%s'" % stage)
    if stage != "test" and data:
        first, last = params.pop("data_cols").split(":")
        data = data[int(first):int(last) if last else None]
    name = params.pop("name")
    if name in _ELSEWHERE:
        raise NotImplementedError("%s is not built here: the cirtorch datasets live in gandtr_amd.mining (tuples, diverse anchors) and "
                                  "gandtr_amd.learning.validation / gandtr_amd.datasets.ImagesFromList (image lists)" % name)
    return DATASET_LABELS[name](data, transform=transform, **params)


def initialize_dataset_loader(data, stage, params, loader_default_params=None, device=None):
    """One ``data:`` block (``transforms``, ``mean_std``, ``dataset``, optional ``loader``) -> ``BatchLoader``.  ``device``: a HIP device (default: the
    current one) builds the chain as a ``DeviceTransform``, a CPU device as the host ``Compose``.  Loader arguments, later ones winning: the defaults
    above, the caller's, the dataset class's, the block's.  Keys nobody consumed are an error."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    chain, mean_std = params.pop("transforms"), params.pop("mean_std")
    if device.type == "cpu":
        transform = initialize_transforms(chain, mean_std=mean_std)
    else:
        from ...ingest import DeviceTransform
        transform = DeviceTransform(chain, mean_std)
    dataset = initialize_dataset(data, stage, transform, params.pop("dataset"))
    settings = dict(LOADER_DEFAULT_PARAMS)
    for layer in (loader_default_params, dataset.loader_params, params.pop("loader", None)):
        settings.update(layer or {})
    assert "batch_size" in settings, "no batch_size in the loader settings"
    assert not params, "unknown keys in the data block: %s" % sorted(params)
    return BatchLoader(dataset, device=device, **settings)
