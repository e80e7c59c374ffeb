"""Model registry (plugin API) -- mirror of mdir/components/model/network/__init__.py:20-48 restricted to the
architectures reachable from the hub entrypoints, the BASELINE configs, the published GAN scenarios' discriminators, CUT's ``featdown`` network, the pix2pix U-Net generator, the learnable photometric normalisation U-Nets (unet.py), the retrieval embedder's attention (``cirnet_attention``) and edge-map
(``cirnet_inchan``) variants and ``normalization_l2``.  Unknown names raise KeyError like the
reference (:48)."""
import torch.nn as nn

from . import cirnet, hed, p2p_networks, rcf, single_layer, unet


class Identity(nn.Module):
    def __init__(self):
        super().__init__()
        self.meta = {"out_channels": 3, "in_channels": 3}

    def forward(self, x):
        return x


MODEL_LABELS = {
    "identity": Identity,
    "official_resnet_generator": p2p_networks.ResnetGenerator,
    "official_p2p_unet_generator": p2p_networks.UnetGenerator,
    "official_p2p_discriminator": p2p_networks.NLayerDiscriminator,
    "official_p2p_mlp": p2p_networks.PatchSampleF,
    "cirnet": cirnet.init_cirnet,
    "cirnet_inchan": cirnet.init_cirnet_inchan,
    "cirnet_attention": cirnet.init_cirnet_attention,
    "normalization_l2": single_layer.NormalizationL2,
    "hed_interpolation": hed.HedInterpolation,
    "rcf": rcf.RCF,
    "p2p_unet": unet.P2pUNet,
    "outconv_unet": unet.OutconvP2pUNet,
    "shallow_p2p_unet": unet.ShallowP2pUNet,
    "inconv_p2p_unet": unet.InconvP2pUNet,
    "aligned_p2p_unet": unet.AlignedP2pUNet,
}


def initialize_model(params):
    return MODEL_LABELS[params.pop("architecture")](**params)
