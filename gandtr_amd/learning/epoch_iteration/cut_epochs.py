"""Step objective of CUT, forward only: mirror of mdir/learning/epoch_iteration/cut_epochs.py, composed from ``patchnce.calculate_nce_loss``."""
import torch

from ...components.optim.criterion import patchnce
from . import gan_epochs
from .gan_epochs import StepLosses, bare_module, call_network


class SupervisedCutEpoch(gan_epochs.SupervisedGanEpoch):
    """CUT (cut_epochs.py:13-89): networks ``generator_X``, ``discriminator_Y``, ``featdown``; criterion a multihead loss with the heads ``adversarial``
    (discriminator_loss), ``identity`` (only its weight is used, as in the reference: the identity term is the patch-NCE loss of ``real_Y`` / ``idt_Y``
    times that weight) and ``nce`` (multilayer_patchnce_loss).  The patch positions of the ``real_X`` / ``fake_Y`` term are drawn first, then the identity
    term's; ``patch_ids=(ids_nce, ids_idt)`` overrides both draws.

    The reference's zero branches (cut_epochs.py:62-72): with an ``nce`` weight of 0 its step fails at ``netG_loss_NCE.total`` (:72), with an ``identity``
    weight of 0 at the logging of ``netG_loss_IDT.total`` (:44) -- there is no logged value to mirror, so both are refused here."""

    def step_losses(self, networks, batch_images, batch_targets, patch_ids=None):
        netG, netD, netF = networks["generator_X"], networks["discriminator_Y"], networks["featdown"]
        crit_nce = self.criterion.losses["nce"]
        w_idt, w_nce = self.criterion.weights["identity"], crit_nce.weight
        if not (w_nce > 0.0 and w_idt > 0.0):
            raise NotImplementedError("the reference's step logs no value when the nce weight (%s) or the identity weight (%s) is 0" % (w_nce, w_idt))
        ids_nce, ids_idt = patch_ids if patch_ids is not None else (None, None)
        with torch.no_grad():
            real_X, real_Y = batch_images, batch_targets
            n = real_X.shape[0]
            fake = call_network(netG, torch.cat((real_X, real_Y), dim=0))
            fake_Y, idt_Y = fake[:n], fake[n:]
            adv = self._adversarial(netD, real_Y, fake_Y)
            # calculate_nce_loss(output, target) of the reference is called as (real_X, fake_Y) and (real_Y, idt_Y): q from the translation, k from the source
            nce = patchnce.calculate_nce_loss(crit_nce, netG, bare_module(netF), real_X, fake_Y, patch_ids=ids_nce)
            idt = patchnce.calculate_nce_loss(crit_nce, netG, bare_module(netF), real_Y, idt_Y, patch_ids=ids_idt)
            assert nce.partial.keys() == idt.partial.keys()
            G_idt = w_idt * idt.total.double()
            G_nce = (w_nce * nce.total.double() + G_idt) * 0.5
            losses = StepLosses([("total", adv.generator + G_nce + adv.discriminator), ("D_real", adv.real), ("D_fake", adv.fake), ("G_gan", adv.generator),
                                 ("G_nce", G_nce), ("G_idt", G_idt)])
            for key in idt.partial:
                losses["G_idt_" + key] = w_idt * idt.partial[key].double()
            for key in nce.partial:
                losses["G_nce_" + key] = (w_nce * nce.partial[key].double() + w_idt * idt.partial[key].double()) * 0.5
            dbg_data = {"real_X": real_X[-1], "real_Y": real_Y[-1], "fake_Y": fake_Y[-1], "idt_Y": idt_Y[-1]}
        return losses, dbg_data
