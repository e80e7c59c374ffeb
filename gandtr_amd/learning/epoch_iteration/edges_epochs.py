"""Step objectives of the edge-consistency scenarios, forward only: mirror of mdir/learning/epoch_iteration/edges_epochs.py.

The detector (HED or RCF) is only asked for its pre-sigmoid maps, ``net(x, no_sigmoid=True)``: the edge-consistency term ``G_hed`` is evaluated from them
with the sigmoid inside ``gdt_map_loss``, the ``dbg_data`` edge maps are ``torch.sigmoid`` of the last image's map."""
import torch

from ...components.optim.criterion import compound
from . import gan_epochs
from .gan_epochs import StepLosses, call_network, map_term


class SupervisedHedGanEpoch(gan_epochs.SupervisedGanEpoch):
    """HED-GAN (edges_epochs.py:4-54): networks ``generator_X``, ``discriminator_Y``, ``detector``; criterion a multihead loss with the heads
    ``adversarial`` (discriminator_loss) and ``edge`` (l1).  Three graph runs: the generator, the discriminator on ``cat[real_Y, fake_Y]``, the detector
    on ``cat[fake_Y, real_X]``."""

    def step_losses(self, networks, batch_images, batch_targets, patch_ids=None):
        netG, netD, netH = networks["generator_X"], networks["discriminator_Y"], networks["detector"]
        with torch.no_grad():
            real_X, real_Y = batch_images, batch_targets
            n = real_X.shape[0]
            fake_Y = call_network(netG, real_X)
            adv = self._adversarial(netD, real_Y, fake_Y)
            maps = call_network(netH, torch.cat([fake_Y, real_X], dim=0), no_sigmoid=True)
            fake_M, real_M = maps[:n], maps[n:]
            hed = map_term(self.criterion, "edge", fake_M, real_M, sigmoid=True)
            G_hed = compound.map_losses([hed]).per_pair[0] * hed.weight
            losses = StepLosses([("total", adv.generator + G_hed + adv.discriminator), ("D_real", adv.real), ("D_fake", adv.fake), ("G_gan", adv.generator),
                                 ("G_hed", G_hed)])
            dbg_data = {"real_X": real_X[-1], "real_Y": real_Y[-1], "fake_Y": fake_Y[-1], "real_E": torch.sigmoid(real_M[-1]),
                        "fake_E": torch.sigmoid(fake_M[-1])}
        return losses, dbg_data


class SupervisedHedNGanEpoch(SupervisedHedGanEpoch):
    """HED-N-GAN (edges_epochs.py:57-121): networks ``generator_X``, ``discriminator_Y``, ``detector`` (the student) and ``detector_frozen`` (the teacher);
    the criterion has a third head ``hed`` (l1) for the distillation terms.  Four graph runs instead of the reference's ten: the generator, the discriminator
    on ``cat[real_Y, fake_Y]``, the teacher on ``real_X``, the student on ``cat[real_X, fake_Y]``; ``E_real``, ``E_fake`` and ``G_hed`` in one ``gdt_map_loss``."""

    def step_losses(self, networks, batch_images, batch_targets, patch_ids=None):
        netG, netD = networks["generator_X"], networks["discriminator_Y"]
        netH_student, netH_teacher = networks["detector"], networks["detector_frozen"]
        with torch.no_grad():
            real_X, real_Y = batch_images, batch_targets
            n = real_X.shape[0]
            fake_Y = call_network(netG, real_X)
            adv = self._adversarial(netD, real_Y, fake_Y)
            target_M = call_network(netH_teacher, real_X, no_sigmoid=True)
            maps = call_network(netH_student, torch.cat([real_X, fake_Y], dim=0), no_sigmoid=True)
            real_M, fake_M = maps[:n], maps[n:]
            terms = [map_term(self.criterion, "hed", real_M, target_M), map_term(self.criterion, "hed", fake_M, target_M),
                     map_term(self.criterion, "edge", fake_M, target_M, sigmoid=True)]
            means = compound.map_losses(terms).per_pair
            E_real, E_fake, G_hed = (means[i] * terms[i].weight for i in range(3))
            losses = StepLosses([("total", adv.generator + G_hed + adv.discriminator), ("D_real", adv.real), ("D_fake", adv.fake), ("G_gan", adv.generator),
                                 ("G_hed", G_hed), ("E_real", E_real), ("E_fake", E_fake)])
            dbg_data = {"real_X": real_X[-1], "real_Y": real_Y[-1], "fake_Y": fake_Y[-1], "real_E": torch.sigmoid(target_M[-1]),
                        "fake_E": torch.sigmoid(fake_M[-1]), "real_E_check": torch.sigmoid(real_M[-1])}
        return losses, dbg_data
