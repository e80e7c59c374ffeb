"""Shared by tests/golden/make_grouping_golden.py, test_grouping_host.py and test_hip_grouping.py: the seeded inputs and the configurations of
tests/golden/grouping.npz (no test in here).  Inputs are regenerated from seeds through gandtr_amd.tools.synth; the fixture stores outputs only."""
import torch

from gandtr_amd.tools import synth

K, D = 7, 16
SIZES = (37, 0, 20)
SEED = 410
GAP = 1e-3                                       # smallest (ma+1)-th minus ma-th squared distance, relative to the ma-th, the generator accepts

# name: (class, features, nearest, assignment, descriptor, weights, extra keyword arguments)
CASES = {
    "normresatt": ("LoadedCodebook", "normresatt", "top-3", "softmax-2.0", "l2norm", "maxassatt", {}),
    "iden": ("LoadedCodebook", "iden", "top", "uniform", "normsign", "unif", {}),
    "resatt": ("LoadedCodebook", "resatt", "top-2", "softmax2-1.5", "sigmoid-3.0", "avgassatt", {}),
    "att": ("LoadedCodebook", "att", "top", "uniform", "l2norm", "descnorm3", {}),
    "soft": ("LoadedCodebook", "normresatt", "all", "softmax-2.0", "l2norm", "maxassatt", {}),
    "batch": ("BatchClustering", "iden", "top", "uniform", "l2norm", "unif", {"clustering": "kmeans", "iterations": 2, "centroids": 5}),
    "topc": ("LoadedCodebook", "normresatt", "top", "uniform", "l2norm", "maxassatt", {"top_centroids": 4}),
}
HARD = ("normresatt", "iden", "resatt", "att")   # fixed codebook, hard assignment: the configurations the device kernels cover end to end
BATCH_SEED = 11


def codebook():
    return synth.synth_input(SEED, (K, D), name="grouping.codebook")


def images(device=None):
    """per image ([features x D], [features x 1]) as ``Grouping._forward`` takes them: 37, 0 and 20 features, half of them close to a centroid"""
    c = codebook()
    out = []
    for i, n in enumerate(SIZES):
        x = synth.synth_input(SEED + 1 + i, (n, D), name="grouping.features")
        if n:
            near = torch.arange(n) % 2 == 0
            x[near] = c[torch.arange(n) % K][near] + 0.4 * x[near]
        att = synth.synth_input(SEED + 11 + i, (n, 1), name="grouping.attention").abs() + 0.1
        out.append(([x.to(device) if device else x], [att.to(device) if device else att]))
    return out


def build(groupings, name, device=None):
    """the layer of case ``name`` from a GROUPINGS table (the reference's or the mirror's)"""
    cls, features, nearest, assignment, descriptor, weights, extra = CASES[name]
    if cls == "BatchClustering":
        return groupings[cls](extra["centroids"], features, nearest, assignment, descriptor, weights, extra["clustering"], extra["iterations"], outputdim=D)
    c = codebook()
    layer = groupings[cls](c.to(device) if device else c, features, nearest, assignment, descriptor, weights, 1.0, extra.get("top_centroids", 0), outputdim=D)
    return layer


def run(layer, name, imgs):
    """(grouped, weights) of ``layer._forward`` on the prepared images, without gradients; the batch clustering draws its Forgy points after
    ``torch.manual_seed(BATCH_SEED)``"""
    if name == "batch":
        torch.manual_seed(BATCH_SEED)
    with torch.no_grad():
        grouped, weights = layer._forward(imgs)
    return grouped, weights
