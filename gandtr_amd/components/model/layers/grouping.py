"""Layers grouping the local descriptors of the images of a tuple over a set of centroids (interface of
mdir/components/model/layers/grouping.py): per image a dense [centroids][dim] descriptor and a weight per centroid.

CPU tensors run the reference's formulas in torch ops.  HIP tensors take the device path (gandtr_amd/codebook.py: nearest centroids without the
distance matrix, ordered segmented sums; inference only, inputs detached) for hard assignment ``top-<ma>`` with ma <= 8, assignment ``uniform`` /
``softmax-b`` / ``softmax2-b`` (the softmax over the ma distances is torch on the [features][ma] result), every feature function except
``normressoftmaxatt``, every descriptor function and every weight function except ``softmaxassatt``.  Everything else on HIP tensors (``all``,
``rankserie``, ``cmeans``, the two softmax-over-features functions, ma > 8, or when a gradient is asked for) runs the torch-op formulation on
the device.  ``maxass`` / ``maxassatt`` on the device path are maxima over the members and 0, which is the reference's dense maximum for the
non-negative assignment weights of these functions."""
import torch

from . import functional

SIZE_SHORTCUTS = {"1k": 1024, "2k": 2048, "4k": 4096, "8k": 8192, "16k": 16384, "32k": 32768,
                  "64k": 65536, "128k": 131072, "256k": 262144, "512k": 524288}

_DEVICE_ASSIGNMENTS = ("uniform", "softmax", "softmax2")
_DEVICE_WEIGHTS = {
    "unif": lambda st, n: (st["max_ass"] != 0).type(torch.float32),
    "maxass": lambda st, n: st["max_ass"],
    "avgass": lambda st, n: st["sum_ass"] / n,
    "maxassatt": lambda st, n: st["max_assatt"],
    "avgassatt": lambda st, n: st["sum_assatt"] / n,
    "avgassatt2": lambda st, n: st["sum_assatt2"] / n,
    "descnorm3": lambda st, n: st["norm"] ** 3,
}


class Grouping(torch.nn.Module):
    """Base class of the groupings"""

    eps = 1e-6

    # hard assignment: x (features, 1, dim), att (features, 1, 1), c (features, ma, dim) -> (features, ma, dim)
    # soft assignment: x (features, 1, dim), att (features, 1, 1), c (centroids, dim) -> (features, centroids, dim)
    feature_functions = {
        "iden": lambda x, att, c: x,
        "att": lambda x, att, c: att * x,
        "res": lambda x, att, c: x - c,
        "resatt": lambda x, att, c: att * (x - c),
        "normres": lambda x, att, c: functional.normalize_vec_l2(x - c),
        "normresatt": lambda x, att, c: att * functional.normalize_vec_l2(x - c),
        "normressoftmaxatt": lambda x, att, c: torch.nn.functional.softmax(att, dim=0) * att * functional.normalize_vec_l2(x - c),
        "normresatt2": lambda x, att, c: att ** 2 * functional.normalize_vec_l2(x - c),
    }

    nearest_params = {
        "all": lambda: None,
        "top": lambda ma=1: ma,
    }

    # dst (features, centroids) -> weights of the same shape
    assignment_functions = {
        "uniform": lambda: (lambda dst: torch.ones_like(dst)),
        "softmax": lambda base, *, detach=False: (lambda dst: functional.assign_weights_softmax(dst.detach() if detach else dst, base)),
        "softmax2": lambda base: (lambda dst: functional.assign_weights_softmax(dst ** 2, base)),
        "rankserie": lambda base: (lambda dst: base ** (-functional.idx2rank_dim1(dst.argsort(dim=1)).type(torch.float32) - 1) * (base - 1)),
        "cmeans": lambda fuzzifier: (lambda dst: functional.assign_weights_cmeans(dst, fuzzifier, 1e-6)),
    }

    # d (centroids, dim) -> the same shape
    descriptor_functions = {
        "l2norm": lambda: (lambda d: d / (torch.norm(d, dim=1, keepdim=True) + 1e-6)),
        "normsign": lambda: (lambda d: torch.sign(d) / d.shape[1] ** 0.5),
        "sigmoid": lambda base: (lambda d: 2 * torch.sigmoid(base * d) - 1),
    }

    # d (centroids, dim), f (features, centroids, dim), att (features, 1), ass (features, centroids) -> (centroids,)
    weight_functions = {
        "unif": lambda: (lambda d, f, att, ass: (ass != 0).any(dim=0).type(torch.float32)),
        "maxass": lambda: (lambda d, f, att, ass: ass.max(dim=0)[0]),
        "avgass": lambda: (lambda d, f, att, ass: ass.mean(dim=0)),
        "maxassatt": lambda *, detach=False: (lambda d, f, att, ass: ((ass * att).detach() if detach else ass * att).max(dim=0)[0]),
        "softmaxassatt": lambda: (lambda d, f, att, ass: (torch.nn.functional.softmax(ass * att, dim=0) * ass * att).sum(dim=0)),
        "avgassatt": lambda *, detach=False: (lambda d, f, att, ass: ((ass * att).detach() if detach else ass * att).mean(dim=0)),
        "avgassatt2": lambda: (lambda d, f, att, ass: (ass * att ** 2).mean(dim=0)),
        "descnorm3": lambda: (lambda d, f, att, ass: torch.norm(d, dim=-1) ** 3),
    }

    def __init__(self, centroids, features, nearest, assignment, descriptor, weights):
        super().__init__()
        centroids = self._parse_size(centroids)
        assert centroids > 0, centroids
        self.feature_function = self.feature_functions[features.lower()]
        self.nearest = self.str_func_call(nearest, self.nearest_params)
        self.assignment_function = self.str_func_call(assignment, self.assignment_functions)
        self.weight_function = self.str_func_call(weights, self.weight_functions)
        self.descriptor_function = self.str_func_call(descriptor, self.descriptor_functions)
        self.params = {"centroids": centroids, "features": features, "nearest": nearest,
                       "assignment": assignment, "descriptor": descriptor, "weights": weights}

    def forward(self, images):
        acc = []
        for feats, atts in images:
            # dim x size1 x size2 maps -> size12 x dim rows
            acc.append(([x.reshape(x.shape[0], -1).T for x in feats], [x.reshape(-1, 1) for x in atts]))
        return self._forward(acc)

    # ---- the device path

    def _device_plan(self, images, centroids):
        """(feature, descriptor, descriptor parameter, weights) names when the HIP kernels cover this configuration and input, else None"""
        from .... import codebook
        p = self.params
        tensors = [centroids] + [x for feats, atts in images for x in list(feats) + list(atts)]
        if not centroids.is_cuda or (torch.is_grad_enabled() and any(t.requires_grad for t in tensors)):
            return None
        if self.nearest is None or not 1 <= self.nearest <= codebook.MAX_MA:
            return None
        descriptor, *dparam = p["descriptor"].lower().split("-")
        names = (p["features"].lower(), descriptor, float(dparam[0]) if dparam else 0.0, p["weights"].lower().split("-")[0])
        if p["assignment"].lower().split("-")[0] not in _DEVICE_ASSIGNMENTS or names[0] not in codebook.FEATURE_FUNCTIONS or names[3] not in _DEVICE_WEIGHTS:
            return None
        return names

    def _assign_images_device(self, images, centroids, plan):
        from .... import codebook
        feature, descriptor, dparam, weights = plan
        centroids = centroids.detach()
        sizes = [sum(f.shape[0] for f in feats) for feats, atts in images]
        if sum(sizes) == 0:
            return (torch.zeros(((len(images),) + centroids.shape), device=centroids.device),
                    torch.zeros((len(images), centroids.shape[0]), device=centroids.device))
        feat = torch.cat([f.detach() for feats, atts in images for f in feats], dim=0).float().contiguous()
        att = torch.cat([a.detach().reshape(-1) for feats, atts in images for a in atts], dim=0).float().contiguous()
        dists, ids = codebook.nearest(feat, centroids, self.nearest)
        ass = self.assignment_function(dists)
        grouped, stats = codebook.aggregate(feat, att, centroids, ids, ass, sizes, feature, descriptor, dparam)
        count = torch.tensor(sizes, dtype=torch.float32).clamp(min=1).to(centroids.device).unsqueeze(1)
        return grouped, _DEVICE_WEIGHTS[weights](stats, count)

    # ---- the torch-op formulation

    def assign_images(self, images, centroids):
        """Every image (all its scales together) on its own"""
        plan = self._device_plan(images, centroids)
        if plan is not None:
            return self._assign_images_device(images, centroids, plan)
        grouped = torch.zeros(((len(images),) + centroids.shape), device=centroids.device)
        weights = torch.zeros((len(images), centroids.shape[0]), device=centroids.device)
        for i, (feats, atts) in enumerate(images):
            feat, att = torch.cat(feats, dim=0), torch.cat(atts, dim=0)
            if feat.shape[0]:
                desc, feat, ass = self.assign_features(feat, att, centroids)
                grouped[i] = self.descriptor_function(desc)
                weights[i] = self.weight_function(desc, feat, att, ass)
        return grouped, weights

    def assign_features(self, features, attentions, centroids):
        """Hard or soft assignment of one image's features: (dense descriptor (centroids, dim), features, dense assignment (features, centroids))"""
        n_feat = features.shape[0]
        if self.nearest is None:
            assignment = self.assignment_function(torch.cdist(features, centroids))
            features = self.feature_function(features.unsqueeze(1), attentions.unsqueeze(1), centroids)
            return (features * assignment.unsqueeze(2)).sum(0), features, assignment

        dists, indexes = torch.topk(torch.cdist(features.detach(), centroids.detach()), self.nearest, dim=1, largest=False, sorted=False)
        assignment = self.assignment_function(dists)
        features = self.feature_function(features.unsqueeze(1), attentions.unsqueeze(1), centroids[indexes])
        descriptor = features * assignment.unsqueeze(2)
        rows = torch.arange(n_feat, device=indexes.device).unsqueeze(1)
        dense_descriptor = torch.zeros(centroids.shape + (n_feat,), device=centroids.device)
        dense_descriptor[indexes, :, rows] = descriptor
        dense_assignment = torch.zeros((n_feat, centroids.shape[0]), device=features.device)
        dense_assignment[rows, indexes] = assignment
        return dense_descriptor.sum(-1), features, dense_assignment

    @staticmethod
    def str_func_call(func, functions):
        """``name-arg1-arg2-flag1`` -> functions[name](arg1, arg2, flag1=True): numeric words are positional arguments (a float when they hold a
        dot), the others are flags"""
        name, *params = func.lower().split("-")
        args, kwargs = [], {}
        for param in params:
            try:
                args.append(float(param) if "." in param else int(param))
            except ValueError:
                kwargs[param] = True
        return functions[name](*args, **kwargs)

    @staticmethod
    def _parse_size(size):
        """"64k" -> 65536"""
        return SIZE_SHORTCUTS[size] if isinstance(size, str) else size

    @staticmethod
    def _detach_flatten(images):
        """All features of all images, detached, as one (features, dim) tensor"""
        return torch.cat([x.detach() for feats, atts in images for x in feats])

    @staticmethod
    def _filter_features(images, feature_mask):
        """Keep the features (and attentions) whose entry of the flat boolean mask is set"""
        pointer, result = 0, []
        for feats, atts in images:
            f_acc, a_acc = [], []
            for f, a in zip(feats, atts):
                mask = feature_mask[pointer:pointer + f.shape[0]]
                f_acc.append(f[mask])
                a_acc.append(a[mask])
                pointer += f.shape[0]
            result.append((f_acc, a_acc))
        assert pointer == feature_mask.shape[0]
        return result

    def __repr__(self):
        return f"{self.__class__.__name__}({', '.join('%s=%s' % (x, y) for x, y in self.params.items())})"


class BatchClustering(Grouping):
    """The centroids are clustered from every batch"""

    clustering_functions = {
        "kmeans": lambda: (lambda f, c, i: functional.iterate_kmeans(f, c, i)),
        "cmeans": lambda fuzzifier: (lambda f, c, i: functional.iterate_cmeans(f, c, i, fuzzifier, 1e-6)),
        "softmax": lambda base: (lambda f, c, i: functional.iterate_softmax(f, c, i, base, 1e-6)),
    }

    def __init__(self, centroids, features, nearest, assignment, descriptor, weights, clustering, iterations, *, outputdim):
        super().__init__(centroids, features, nearest, assignment, descriptor, weights)
        self.clustering = self.str_func_call(clustering, self.clustering_functions)
        self.params.update({"clustering": clustering, "iterations": iterations})

    def _forward(self, images):
        features = self._detach_flatten(images)
        clusters = functional.init_clusters_forgy(features, self.params["centroids"])
        clusters = self.clustering(features, clusters, self.params["iterations"])
        return self.assign_images(images, clusters)


class Codebook(Grouping):
    """Base class of the codebook groupings (large codebooks, e.g. 64k centroids)"""

    def __init__(self, codebook, features, nearest, assignment, descriptor, weights, lr_multiplier, top_centroids):
        super().__init__(len(codebook), features, nearest, assignment, descriptor, weights)
        self.codebook = torch.nn.Parameter(codebook)
        self.lr_multiplier = lr_multiplier
        self.top_centroids = self._parse_size(top_centroids)
        if self.top_centroids:
            assert [x for x in ["max", "sum", "avg", "unif"] if self.params["weights"].lower().startswith(x)], self.params["weights"]

    def _forward(self, images):
        codebook = self.codebook
        if self.top_centroids:
            pospair = images[:2]                                   # the weights come from the query and the positive only
            atts = torch.cat([x.detach() for feats, atts in pospair for x in atts])
            if self.nearest is None:
                features = self._detach_flatten(pospair)
                weights = self._chunk_weights_all(features, atts, codebook.detach(), 1_000_000)
                codebook = codebook[weights.topk(self.top_centroids, largest=True, sorted=False)[1]]
            else:
                assert self.nearest == 1, "ma with chunking not implemented"
                features = self._detach_flatten(images)            # every image's features are assigned
                wgt, ass = self._chunk_weights_topk(features, atts, codebook.detach(), 1_000_000)
                codebook, feature_mask = self._reduce_codebook(wgt, ass, codebook, self.top_centroids)
                if feature_mask is not None:
                    images = self._filter_features(images, feature_mask)
        return self.assign_images(images, codebook)

    @staticmethod
    def _block_slices(n_features, n_centroids, block_size):
        step = max(block_size // n_centroids, 1) if block_size is not None else n_features
        starts = list(range(0, n_features, step))
        return list(zip(starts, starts[1:] + [n_features]))

    def _chunk_weights_topk(self, features, atts, codebook, block_size):
        """Centroid weights and the arg-min assignment in blocks of ``block_size`` distances.  On HIP tensors the arg-min of ALL features is one
        gdt_codebook_nearest call (no distance block exists); the weights keep the reference's block structure."""
        n_features = features.shape[0]
        slices = self._block_slices(n_features, codebook.shape[0], block_size)
        if features.is_cuda:
            from .... import codebook as device
            assignment = device.nearest(features, codebook, 1)[1].reshape(-1).long()
        else:
            assignment = torch.empty(n_features, device=codebook.device, dtype=torch.int64)
            for start, end in slices:
                assignment[start:end] = torch.cdist(features[start:end], codebook).argmin(dim=1)
        weights = torch.zeros(len(slices), codebook.shape[0], device=codebook.device)
        for i, (start, end) in enumerate(slices):
            if atts.shape[0] <= start:
                continue
            idx = assignment[start:min(end, atts.shape[0])]
            ass = torch.zeros(idx.shape[0], codebook.shape[0], device=codebook.device)
            ass[torch.arange(idx.shape[0], device=idx.device), idx] = 1
            weights[i] = self.weight_function(None, None, atts[start:end], ass)
        return self._reduce_slices(weights, slices, self.params["weights"]), assignment

    def _chunk_weights_all(self, features, atts, codebook, block_size):
        """Centroid weights of the soft assignment in blocks of ``block_size`` distances"""
        slices = self._block_slices(features.shape[0], codebook.shape[0], block_size)
        weights = torch.zeros(len(slices), codebook.shape[0], device=codebook.device)
        for i, (start, end) in enumerate(slices):
            ass = self.assignment_function(torch.cdist(features[start:end], codebook))
            weights[i] = self.weight_function(None, None, atts[start:end], ass)
        return self._reduce_slices(weights, slices, self.params["weights"])

    @staticmethod
    def _reduce_slices(result, slices, reduction):
        """Join the per-block weights by the weight function's own reduction (max, sum, avg)"""
        reduction = reduction.lower()
        if reduction.startswith("max") or reduction.startswith("unif"):
            return result.max(dim=0)[0]
        if reduction.startswith("sum"):
            return result.sum(dim=0)
        if reduction.startswith("avg"):
            sizes = torch.tensor([y - x for x, y in slices], device=result.device)
            return (result * sizes.unsqueeze(1)).sum(dim=0) / sizes.sum()

    @staticmethod
    def _reduce_codebook(weights, assignment, codebook, top_centroids):
        """Keep the ``top_centroids`` heaviest centroids; the mask drops the features assigned to the others"""
        nonzero = weights > 0
        if nonzero.sum() < top_centroids:
            return codebook[nonzero], None
        idx = weights[nonzero].argsort(descending=True)
        idx = torch.arange(nonzero.shape[0], device=nonzero.device)[nonzero][idx]      # back to codebook indices
        codebook = codebook[idx[:top_centroids]]
        exclude = idx[top_centroids:].to(assignment.device)
        return codebook, (assignment.unsqueeze(1) != exclude).all(dim=1)


class ClusteringCodebook(Codebook):
    """The codebook is clustered once, at the beginning of the first epoch"""

    recompute = False

    def __init__(self, centroids, features, nearest, assignment, descriptor, weights, lr_multiplier, top_centroids, iterations, *, outputdim,
                 **inference_params):
        super().__init__(torch.zeros((self._parse_size(centroids), outputdim)), features, nearest, assignment, descriptor, weights, lr_multiplier,
                         top_centroids)
        self.params["iterations"] = iterations
        self.inference_params = inference_params

    def compute_codebook(self, descriptors):
        """The reference calls a ``self.clustering`` that it never sets (an AttributeError there); here the codebook is Forgy initialisation +
        ``functional.iterate_kmeans`` for ``iterations`` iterations."""
        centroids = functional.init_clusters_forgy(descriptors.detach(), self.params["centroids"]).clone()
        self.codebook.data = functional.iterate_kmeans(descriptors.detach(), centroids, self.params["iterations"])


class LoadedCodebook(Codebook):
    """A codebook trained elsewhere"""

    def __init__(self, centroids, features, nearest, assignment, descriptor, weights, lr_multiplier, top_centroids, *, outputdim):
        super().__init__(self.load_codebook(centroids), features, nearest, assignment, descriptor, weights, lr_multiplier, top_centroids)

    @staticmethod
    def load_codebook(path):
        """A tensor, or the path of a pickle ``{"state": {"centroids": ndarray}}``, read through the restricted unpickler of tools/utils.py
        (containers and numpy arrays only)"""
        if isinstance(path, torch.Tensor):
            return path
        from ....tools import utils
        return torch.from_numpy(utils.fs_load_pickle(path)["state"]["centroids"])


class FaissCodebook(Codebook):
    """The reference clusters this codebook with faiss (``asmk``); here ``compute_codebook`` raises ImportError"""

    recompute = False

    def __init__(self, centroids, features, nearest, assignment, descriptor, weights, lr_multiplier, top_centroids, *, outputdim, **inference_params):
        super().__init__(torch.zeros((self._parse_size(centroids), outputdim)), features, nearest, assignment, descriptor, weights, lr_multiplier,
                         top_centroids)
        self.inference_params = inference_params

    def compute_codebook(self, descriptors):
        self.codebook.data = functional.cluster_faiss(descriptors, self.params["centroids"])


GROUPINGS = {
    "BatchClustering": BatchClustering,
    "ClusteringCodebook": ClusteringCodebook,
    "LoadedCodebook": LoadedCodebook,
    "FaissCodebook": FaissCodebook,
}
