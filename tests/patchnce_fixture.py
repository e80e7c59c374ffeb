"""Shared by test_patchnce_host.py and test_hip_patchnce.py: the cases of tests/golden/patchnce.npz rebuilt from their seeds (no test in here)."""
import os

import numpy as np
import torch

from gandtr_amd.tools import synth

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patchnce.npz"))
N_HEAD, N_PIPE = int(GOLD["n_head_cases"]), int(GOLD["n_pipe_cases"])
TEMPERATURE, WEIGHT = float(GOLD["temperature"]), float(GOLD["weight"])
NCE_LAYERS = str(GOLD["nce_layers"])
PIPE_PATCHES = int(GOLD["pipe_patches"])


def head_case(i):
    """(PatchSampleF mirror in eval mode with the fixture's seeded weights, q map, k map, (B, C, H, W, P, nc), fixture prefix); nc 0 = use_mlp off"""
    from gandtr_amd.components.model.network import p2p_networks
    p = "h%d_" % i
    B, C, H, W, P, nc = (int(v) for v in GOLD[p + "shape"])
    qmap, kmap = synth.patchnce_maps(70 + i, (B, C, H, W))
    netF = p2p_networks.PatchSampleF(use_mlp=nc > 0, input_nc=None, nc=nc or 256, nce_layers=None)
    if nc:
        netF.create_mlp([kmap], "cpu")
        netF.load_state_dict(synth.patchsample_state(60 + i, [C], nc))
    return netF.eval(), qmap, kmap, (B, C, H, W, P, nc), p


def pipe_case(i):
    """(generator, featdown, src, tgt, stored ids per layer, fixture prefix): the 9-block InstanceNorm generator with layers 4,8,12,16"""
    from gandtr_amd.components.model.network import p2p_networks
    p = "p%d_" % i
    shape = tuple(int(v) for v in GOLD[p + "shape"])
    netG = p2p_networks.ResnetGenerator(3, 3, norm_layer="instance").eval()
    netG.load_state_dict(synth.generator_state(0, "instance"))
    netF = p2p_networks.PatchSampleF(input_nc=3, nc=256, nce_layers=NCE_LAYERS).eval()
    netF.load_state_dict(synth.patchsample_state(90, (128, 256, 256, 256), 256))
    src, tgt = synth.synth_input(91 + i, shape, 1.0, name="src"), synth.synth_input(91 + i, shape, 1.0, name="tgt")
    ids = [torch.from_numpy(GOLD[p + "ids%d" % l].astype(np.int64)) for l in range(4)]
    return netG, netF, src, tgt, ids, p


def criterion(groups, layers=NCE_LAYERS, num_patches=PIPE_PATCHES):
    from gandtr_amd.components.optim.criterion import patchnce
    return patchnce.initialize_patchnce_criterion({"loss": "multilayer_patchnce_loss", "batch_dim_for_bmm": groups, "nce_layers": layers,
                                                   "num_patches": num_patches, "temperature": TEMPERATURE, "weight": WEIGHT})
