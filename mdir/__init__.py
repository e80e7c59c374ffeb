"""Drop-in alias: ``import mdir...`` resolves to the MI355X host mirror in ``gandtr_amd`` for the modules on the hot path.

    mdir.hub.model                         -> gandtr_amd.hub.model
    mdir.components.model.network          -> gandtr_amd.components.model.network   (MODEL_LABELS, initialize_model)
    mdir.components.model.network.unet     -> gandtr_amd.components.model.network.unet (P2pUNet, OutconvP2pUNet, InconvP2pUNet, AlignedP2pUNet, ShallowP2pUNet)
    mdir.components.model.layers(.attention|.pooling|.preprocessing) -> gandtr_amd.components.model.layers (ATTENTIONS, L2NormAttention, POOLINGS, GeometricMedianWeiszfeld, EdgeFilter)
    mdir.components.model.layers(.grouping|.functional) -> gandtr_amd.components.model.layers (GROUPINGS, BatchClustering, LoadedCodebook, iterate_kmeans, ..)
    mdir.components.data.wrapper           -> gandtr_amd.components.data.wrapper    (WRAPPERS_LABELS, initialize_wrappers)
    mdir.components.data.transform         -> gandtr_amd.components.data.transform  (initialize_transforms)
    mdir.components.data.dataset           -> gandtr_amd.components.data.dataset    (DATASET_LABELS, initialize_dataset_loader: the GAN scenarios' data)
    mdir.learning / mdir.learning.network  -> gandtr_amd.learning(.network)         (NETWORKS, initialize_network, load_network)
    mdir.learning.validation               -> gandtr_amd.learning.validation        (initialize_validation, SingleValidation, ...)
    mdir.components.optim.score            -> gandtr_amd.components.optim.score     (SCORES, initialize_score: cirdatasetap)
    mdir.components.optim.criterion        -> gandtr_amd.components.optim.criterion (CRITERIA, initialize_criterion: contrastive, triplet)
    mdir.components.optim.criterion.adversarial -> gandtr_amd.components.optim.criterion.adversarial (DiscriminatorLoss, patch_scores)
    mdir.components.optim.criterion.patchnce -> gandtr_amd.components.optim.criterion.patchnce (MultilayerPatchNCELoss, calculate_nce_loss)
    mdir.components.optim.criterion.compound -> gandtr_amd.components.optim.criterion.compound (GAN_CRITERIA, initialize_gan_criterion: l1, mse, multihead_loss, ..)
    mdir.learning.epoch_iteration          -> gandtr_amd.learning.epoch_iteration   (EPOCH_ITERATIONS: the GAN scenarios' step_losses; gan_epochs, edges_epochs, cut_epochs)
    mdir.stages.infer                      -> gandtr_amd.stages.infer               (infer(params, data))
    mdir.stages.multistep                  -> gandtr_amd.stages.multistep           (infer_and_learn_whitening(params, data))
    mdir.tools.tensors                     -> gandtr_amd.tools.tensors

Unlike the reference's ``mdir/__init__.py`` this does NOT call ``torch.set_num_threads(3)`` (mdir/stages/infer.py:12-15)
and does not touch ``sys.path``; set ``GANDTR_REFERENCE_THREADS=1`` to reproduce the thread cap.
"""
import importlib
import os
import sys

_ALIASES = {
    "mdir.hub": "gandtr_amd.hub",
    "mdir.hub.model": "gandtr_amd.hub.model",
    "mdir.components": "gandtr_amd.components",
    "mdir.components.model": "gandtr_amd.components.model",
    "mdir.components.model.network": "gandtr_amd.components.model.network",
    "mdir.components.model.layers": "gandtr_amd.components.model.layers",
    "mdir.components.model.layers.attention": "gandtr_amd.components.model.layers.attention",
    "mdir.components.model.layers.pooling": "gandtr_amd.components.model.layers.pooling",
    "mdir.components.model.layers.preprocessing": "gandtr_amd.components.model.layers.preprocessing",
    "mdir.components.model.layers.grouping": "gandtr_amd.components.model.layers.grouping",
    "mdir.components.model.layers.functional": "gandtr_amd.components.model.layers.functional",
    "mdir.components.model.network.single_layer": "gandtr_amd.components.model.network.single_layer",
    "mdir.components.model.network.p2p_networks": "gandtr_amd.components.model.network.p2p_networks",
    "mdir.components.model.network.cirnet": "gandtr_amd.components.model.network.cirnet",
    "mdir.components.model.network.hed": "gandtr_amd.components.model.network.hed",
    "mdir.components.model.network.rcf": "gandtr_amd.components.model.network.rcf",
    "mdir.components.model.network.unet": "gandtr_amd.components.model.network.unet",
    "mdir.components.model.weight_initialization": "gandtr_amd.components.model.weight_initialization",
    "mdir.components.data": "gandtr_amd.components.data",
    "mdir.components.data.wrapper": "gandtr_amd.components.data.wrapper",
    "mdir.components.data.transform": "gandtr_amd.components.data.transform",
    "mdir.components.data.dataset": "gandtr_amd.components.data.dataset",
    "mdir.learning": "gandtr_amd.learning",
    "mdir.learning.network": "gandtr_amd.learning.network",
    "mdir.learning.checkpoints": "gandtr_amd.learning.checkpoints",
    "mdir.learning.validation": "gandtr_amd.learning.validation",
    "mdir.components.optim": "gandtr_amd.components.optim",
    "mdir.components.optim.score": "gandtr_amd.components.optim.score",
    "mdir.components.optim.score.cirscore": "gandtr_amd.components.optim.score.cirscore",
    "mdir.components.optim.criterion": "gandtr_amd.components.optim.criterion",
    "mdir.components.optim.criterion.adversarial": "gandtr_amd.components.optim.criterion.adversarial",
    "mdir.components.optim.criterion.patchnce": "gandtr_amd.components.optim.criterion.patchnce",
    "mdir.components.optim.criterion.compound": "gandtr_amd.components.optim.criterion.compound",
    "mdir.learning.epoch_iteration": "gandtr_amd.learning.epoch_iteration",
    "mdir.learning.epoch_iteration.gan_epochs": "gandtr_amd.learning.epoch_iteration.gan_epochs",
    "mdir.learning.epoch_iteration.edges_epochs": "gandtr_amd.learning.epoch_iteration.edges_epochs",
    "mdir.learning.epoch_iteration.cut_epochs": "gandtr_amd.learning.epoch_iteration.cut_epochs",
    "mdir.stages": "gandtr_amd.stages",
    "mdir.stages.infer": "gandtr_amd.stages.infer",
    "mdir.stages.whiten": "gandtr_amd.stages.whiten",
    "mdir.stages.multistep": "gandtr_amd.stages.multistep",
    "mdir.stages.validate": "gandtr_amd.stages.validate",
    "mdir.tools": "gandtr_amd.tools",
    "mdir.tools.tensors": "gandtr_amd.tools.tensors",
    "mdir.tools.utils": "gandtr_amd.tools.utils",
}

for _alias, _target in _ALIASES.items():
    _mod = importlib.import_module(_target)
    sys.modules[_alias] = _mod
    _parent, _, _leaf = _alias.rpartition(".")
    setattr(sys.modules[_parent], _leaf, _mod)

if os.environ.get("GANDTR_REFERENCE_THREADS") == "1":
    import torch
    torch.set_num_threads(3)
