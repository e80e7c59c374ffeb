"""mirror of mdir/learning/validation.py:11-165: the validation tasks of a scenario's ``validation`` section.

``data: null``: the criterion is a score of the network (``cirdatasetap``).  ``data: <key>``: the loss validation of the fine-tuning scenario
(mdir/examples/iccv23/parameters/finetune.yml:61-66, :90-102) -- the criterion is a loss over the tuples mined from ``params_data[key]``'s
tuple dataset (``CirTuples`` / ``CirDiverseAnchors``).  The reference reads that dataset from disk and scores one tuple per iteration (seven
batch-1 forwards, a criterion call and an ``.item()`` each, validation.py:93-107); here ``data`` carries the dataset in memory, every distinct
image of the mined tuples is embedded ONCE through the batched extractor and all tuple losses come from one launch over an index table
(``TuplesData``, ``SingleValidation.validate``).  Any validation type other than SingleValidation / MultiCriterialValidation raises
NotImplementedError."""
import copy
import os
import time

import torch

from .. import mining
from ..components.optim.criterion import initialize_criterion
from ..components.optim.score import initialize_score

_DATASET_KEYS = {"dataset", "dataset_pkl", "image_dir", "image_size", "name", "neg_num", "pool_size", "query_size", "split",
                 "qpool_size", "similar_exclude", "similar_include", "mark_easy", "shuffle", "first_neg"}


class TuplesData:
    """The tuple dataset of a loader-based validation, in memory: what ``initialize_dataset_loader(data, "val", params)`` builds from disk
    (mdir/components/data/dataset/cirtorch_datasets.py:7-30).  ``data = {"db": <the dict the reference unpickles for this split: qidxs,
    pidxs, cluster, optionally cids>, "images": <per image index a file path, file contents or an already transformed C x H x W tensor>,
    "names": <optional, per image index the name the loader would report>}``.  ``params``: ``{"dataset": {finetune.yml:91-102}, "loader":
    {"batch_size": 1}}`` merged over the network's ``runtime.data`` (``mean_std``, ``transforms``).  ``dataset`` / ``dataset_pkl`` /
    ``image_dir`` / ``split`` name what ``data`` already holds and are not read.  An image's name is ``names[i]``, else ``db["cids"][i]``
    (the reference's files are named by cid), else a path's base name without extension, else the index."""

    def __init__(self, data, params):
        if not isinstance(data, dict) or not {"db", "images"} <= data.keys():
            raise ValueError('a loader-based validation takes data = {"db": ..., "images": [...]} in memory')
        params = dict(params)
        dataset = dict(params.pop("dataset"))
        loader = dict(params.pop("loader", None) or {})
        if loader.pop("batch_size", 1) != 1 or loader:
            raise NotImplementedError("a loss validation scores one tuple per iteration (loader batch_size 1), as finetune.yml")
        self.mean_std, self.transforms = params.pop("mean_std", None), params.pop("transforms", None)
        assert not params, params.keys()
        unknown = dataset.keys() - _DATASET_KEYS
        assert not unknown, unknown
        self.db, self.images, self.names = data["db"], data["images"], data.get("names")
        self.name = dataset["name"]
        if self.name not in ("CirTuples", "CirDiverseAnchors"):
            raise NotImplementedError("validation dataset %r is not provided by this build (available: CirTuples, CirDiverseAnchors)" % (self.name,))
        self.image_size = dataset["image_size"]
        self.first_neg = dataset.get("first_neg", "neg")
        if self.first_neg != "neg":
            raise NotImplementedError("first_neg = %r: the tuple loss takes (anchor, positive, negatives..) tuples" % (self.first_neg,))
        self.mining = dict(qsize=dataset["query_size"], poolsize=dataset["pool_size"], nnum=dataset["neg_num"], shuffle=dataset.get("shuffle", True),
                           first_neg=self.first_neg, name=self.name)
        if self.name == "CirDiverseAnchors":
            self.mining.update(qpool_size=dataset["qpool_size"], similar_exclude=dataset["similar_exclude"],
                               similar_include=dataset["similar_include"], mark_easy=dataset.get("mark_easy"))
        self.qsize = min(mining._all_or(dataset["query_size"], len(self.db["qidxs"])), len(self.db["qidxs"]))
        self.qidxs = self.pidxs = self.nidxs = self.tuple_labels = None

    def __len__(self):
        return self.qsize

    def image_name(self, i):
        if self.names is not None:
            return str(self.names[i])
        if "cids" in self.db:
            return str(self.db["cids"][i])
        if isinstance(self.images[i], (str, os.PathLike)):
            return os.path.basename(os.fspath(self.images[i])).rsplit(".", 1)[0]
        return str(i)

    def extract(self, network, device, idxs, labels):
        """D x len(idxs) descriptors of the images ``idxs`` under the image labels ``labels`` (one for all, or one each), equal-sized images
        batched (stages.validate.extract_vectors); files are decoded, resized to ``image_size`` and transformed on the device."""
        from .. import jpeg
        from ..ingest import DeviceTransform
        from ..stages.validate import extract_vectors
        labels = [labels] * len(idxs) if isinstance(labels, str) else list(labels)
        meta = [{"image_label": l, "name": self.image_name(i)} for i, l in zip(idxs, labels)]
        cols, chunk = [], 64
        for lo in range(0, len(idxs), chunk):
            items = [self.images[i] for i in idxs[lo:lo + chunk]]
            files = [k for k, x in enumerate(items) if not torch.is_tensor(x)]
            if files:
                if self.mean_std is None or self.transforms is None:
                    raise ValueError("image files need runtime.data.mean_std and transforms in the network parameters")
                tr = DeviceTransform(self.transforms, self.mean_std)
                mean, std = (tr.mean, tr.std) if tr.normalize else ([0.0] * 3, [1.0] * 3)
                decoded = jpeg.ingest_files([items[k] for k in files], self.image_size, mean, std, clahe_clip=tr.clahe_clip, clahe_grid=tr.clahe_grid,
                                            device=device)
                for k, t in zip(files, decoded):
                    items[k] = t
            cols.append(extract_vectors(network, items, device, metadata=meta[lo:lo + chunk]))
        return torch.cat(cols, dim=1)

    def prepare_epoch(self, network, device):
        """``create_epoch_tuples`` (traindataset.py:281-303); the descriptors it mines with carry the reference's ``-mine`` image labels"""
        def extract(idxs, label):
            mine = label + "-mine" if isinstance(label, str) else ["%s-mine" % x for x in label]
            return self.extract(network, device, [int(i) for i in idxs], mine)
        self.qidxs, self.pidxs, self.nidxs, self.tuple_labels, meta = mining.create_epoch_tuples(
            self.db, self.images, network, self.image_size, self.mean_std, extract=extract, **self.mining)
        return meta

    def __repr__(self):
        return "%s (name: %s, images: %d, pairs: %d, mining: %s)" % (type(self).__name__, self.name, len(self.images), len(self.db["qidxs"]), self.mining)


class NoValidation:

    def __init__(self, decisive_criterion=""):
        self.decisive_criterion = decisive_criterion

    def validations(self, _epoch):
        return []

    def should_validate(self, _epoch):
        return False

    def __repr__(self):
        return "%s ()" % type(self).__name__


class SingleValidation:

    def __init__(self, criterion, network_overlay, frequency, decisive_criterion, data_loader=None, criterion_mean_reduction=None):
        self.data_loader = data_loader                    # a TuplesData (there is no DataLoader: the tuples are scored from an index table)
        self.criterion = criterion
        self.network_overlay = network_overlay
        self.frequency = frequency
        self.decisive_criterion = decisive_criterion
        self.criterion_mean_reduction = criterion_mean_reduction

    @classmethod
    def initialize(cls, params_validation, data=None, params_data=None, default_criterion=None, network=None):
        net_defaults = network.network_params.runtime.get("data", {}) if network is not None else {}
        data_key = params_validation.pop("data")
        data_loader = None
        if data_key is not None:
            if data is None or not params_data or data_key not in params_data:
                raise NotImplementedError("validation data %r: a loader-based (loss) validation is built from in-memory data -- data = {\"db\": ..., "
                                          "\"images\": [...]} and the dataset's definition in params_data[%r]; reading datasets from disk is "
                                          "not provided by this build" % (data_key, data_key))
            data_loader = TuplesData(data, copy.deepcopy({**net_defaults, **params_data[data_key]}))
        criterion_section = params_validation.pop("criterion")
        if criterion_section == "default":
            if default_criterion is None:
                raise ValueError("Criterion cannot be 'default' when default criterion is not specified")
            criterion = default_criterion
        elif data_loader is None:
            criterion = initialize_score(copy.deepcopy({**net_defaults, **criterion_section}))
        else:
            criterion = initialize_criterion(copy.deepcopy(criterion_section))
        network_overlay = params_validation.pop("network_overlay")
        frequency = params_validation.pop("frequency")
        assert not params_validation, params_validation.keys()
        if data_loader is None:
            return cls(criterion=criterion, network_overlay=network_overlay, frequency=frequency,
                       decisive_criterion=criterion.decisive_criterion)
        assert criterion.reduction in {"mean", "sum"}, criterion.reduction
        if not hasattr(criterion, "tuple_losses"):
            raise NotImplementedError("a loss validation needs a tuple criterion (contrastive, triplet), got %r" % (criterion,))
        return cls(criterion=criterion, network_overlay=network_overlay, frequency=frequency, decisive_criterion="val/learning/loss:total",
                   data_loader=data_loader, criterion_mean_reduction=criterion.reduction == "mean")

    def validations(self, epoch):
        return [("val", self)] if self.should_validate(epoch) else []

    def should_validate(self, epoch):
        return epoch is None or bool(self.frequency and (epoch + 1) % self.frequency == 0)

    def validate(self, network, device, logger):
        if self.network_overlay:
            network = network.overlay_params(copy.deepcopy(self.network_overlay), device)
        network.eval()
        if self.data_loader is None:
            return self.criterion(network, device, logger)
        return self._validate_tuples(network, device, logger)

    def _validate_tuples(self, network, device, logger):
        """validation.py:86-109 on the whole epoch at once: mine the tuples, embed every distinct (image, image label) once, score all tuples
        in one launch; the losses come back to the host once, as the list the reference accumulates"""
        val, start = self.data_loader, time.time()
        with torch.no_grad():
            metadata = val.prepare_epoch(network, device)
            mined = time.time()
            if metadata:
                logger(None, len(val), "data_mining", metadata, "scalar/loss")
            logger(None, len(val), "prepare_epoch", {"prepare_data": mined - start}, "scalar/time")
            entries, table = mining.epoch_tuple_table(val.qidxs, val.pidxs, val.nidxs, val.tuple_labels)
            vecs = val.extract(network, device, [i for i, _ in entries], [label for _, label in entries])
            losses = self.criterion.tuple_losses(vecs, table).loss
            # a batch is one tuple (loader batch_size 1): a "sum" criterion is reported per batch element, a "mean" one as it is
            batch_len = 1
            acc = [float(x) if self.criterion_mean_reduction else float(x) / batch_len for x in losses.cpu().tolist()]
        for i, loss in enumerate(acc):
            logger(i, len(val), "loss", {"total": loss}, "scalar/loss")
        logger(None, len(val), "iteration", {"process_epoch": time.time() - mined}, "scalar/time")
        return acc

    def __repr__(self):
        if self.data_loader is None:
            return "%s (criterion: %s, network_overlay: %s, frequency: %s, decisive_criterion: %s)" % (
                type(self).__name__, self.criterion, self.network_overlay, self.frequency, self.decisive_criterion)
        return "%s (dataset: %s, criterion: %s, network_overlay: %s, frequency: %s, decisive_criterion: %s, criterion_mean_reduction: %s)" % (
            type(self).__name__, self.data_loader, self.criterion, self.network_overlay, self.frequency, self.decisive_criterion,
            self.criterion_mean_reduction)


class MultiCriterialValidation:

    def __init__(self, decisive_criterion, validations):
        self.decisive_criterion = decisive_criterion
        self.vals = validations

    @classmethod
    def initialize(cls, params_validation, **kwargs):
        decisive_criterion = params_validation.pop("decisive_criterion")
        validations = {key: initialize_validation(scenario, **kwargs) for key, scenario in params_validation.items()}
        return cls(decisive_criterion, validations)

    def validations(self, epoch):
        return [(key, val) for key, val in self.vals.items() if val.should_validate(epoch)]

    def __repr__(self):
        return "%s (decisive_criterion: %s, validations: %s)" % (type(self).__name__, self.decisive_criterion,
                                                                 ", ".join("%s: %s" % kv for kv in self.vals.items()))


VALIDATIONS = {
    "SingleValidation": SingleValidation,
    "MultiCriterialValidation": MultiCriterialValidation,
}


def initialize_validation(params, **kwargs):
    if isinstance(params, bool) and not params:
        return NoValidation()
    if isinstance(params, str):
        return NoValidation(params)
    kind = params.pop("type", None)
    if kind not in VALIDATIONS:
        raise NotImplementedError("validation type %r is not provided by this build (available: %s)" % (kind, ", ".join(VALIDATIONS)))
    return VALIDATIONS[kind].initialize(params, **kwargs)
