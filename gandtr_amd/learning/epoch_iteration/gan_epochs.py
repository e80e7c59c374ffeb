"""Step objectives of the GAN scenarios, forward only: mirror of mdir/learning/epoch_iteration/gan_epochs.py.

``step_losses(networks, batch_images, batch_targets)`` returns what the reference's ``_optimization_step`` logs when every optimizer is a no-op and every
network is in ``.eval()``: the same keys in the same order.  Because nothing updates between the reference's sub-steps, a network's repeated forwards of one
input are computed once, and forwards of the same network on several inputs run as ONE concatenated batch (InstanceNorm and eval-mode BatchNorm act per
image).  The terms come from ``gdt_patch_score`` (discriminator side) and ``gdt_map_loss`` (l1 / mse heads); nothing returns to the host until
``StepLosses.item()`` brings every value over in one transfer."""
from collections import OrderedDict

import torch

from ...components.optim.criterion import adversarial, compound
from ...components.optim.criterion.compound import initialize_gan_criterion


class StepLosses(OrderedDict):
    """the logged losses of one step: key -> 0-dim tensor on the inputs' device (float64 on a HIP device)"""

    def item(self):
        """the same keys -> Python floats, with ONE transfer to the host"""
        values = torch.stack([v.detach().double() for v in self.values()]).cpu().tolist() if self else []
        return OrderedDict(zip(self.keys(), values))


def call_network(net, x, **params):
    """a ``learning.network.Network`` goes through its ``forward`` (wrappers included), a bare module is called"""
    from ..network import Network
    return net.forward(x, **params) if isinstance(net, Network) else net(x, **params)


def bare_module(net):
    from ..network import Network
    return net.model if isinstance(net, Network) else net


def _map_criterion(criterion, key):
    crit = criterion.losses[key]
    if not isinstance(crit, compound._MapLoss) or crit.reduction == "none":
        raise NotImplementedError("the %r head is an l1 / mse criterion with a reduction here, got %r" % (key, crit))
    return crit, criterion.weights[key]


def map_term(criterion, key, a, b, sigmoid=False):
    """the MapPair of head ``key`` of a MultiheadLoss, weighted with its weight (reduction "sum": times the number of values)"""
    crit, w = _map_criterion(criterion, key)
    return crit.pairs(a, b, weight=w * (a.numel() if crit.reduction == "sum" else 1), sigmoid=sigmoid)


class AdversarialScores:
    """the adversarial terms of ONE discriminator forward on ``cat[real, fake]``: ``w * criterion(pred_real, True)``, ``w * criterion(pred_fake, False)`` and
    the generator's ``w * criterion(pred_fake, True)`` -- DiscriminatorLoss's quirk included (the target is ``int(not is_target_real)``).  The discriminator is
    reached the way the reference's step reaches it: ``netD.forward(..)`` through the network object, wrappers included (gan_epochs.py:36-37, the HED and CUT
    steps), or, with ``multi``, ``netD.model.forward_multi(..)`` on the bare model (gan_epochs.py:132-133, CycleGAN's discriminator step)"""

    def __init__(self, criterion, weight, netD, real, fake, multi=False):
        if not isinstance(criterion, adversarial.DiscriminatorLoss):
            raise NotImplementedError("the adversarial head is a discriminator_loss, got %r" % (criterion,))
        both = torch.cat([real, fake], dim=0)
        pred = bare_module(netD).forward_multi(both) if multi else call_network(netD, both)
        if isinstance(pred, list):
            raise NotImplementedError("multiscale discriminators are not provided by this build")
        scores = adversarial.patch_scores(pred, criterion.kind)
        per_target = (scores.loss_target0, scores.loss_target1)
        n = real.shape[0]
        self.pred_fake = pred[n:]
        self.real = weight * per_target[criterion.get_target(True)][:n].mean()
        self.fake = weight * per_target[criterion.get_target(False)][n:].mean()
        self.generator = weight * per_target[criterion.get_target(True)][n:].mean()
        self.discriminator = (self.real + self.fake) * 0.5


class SupervisedGanEpoch:
    """Base of the GAN step objectives: holds the criterion"""

    def __init__(self, criterion):
        self.criterion = criterion

    @classmethod
    def initialize(cls, params_epoch, default_criterion=None, **_unused):
        params_epoch = dict(params_epoch)
        params_epoch.pop("data", None)
        section = params_epoch.pop("criterion", "default")
        if section == "default":
            if default_criterion is None:
                raise ValueError("Criterion cannot be 'default' when default criterion is not specified")
            criterion = default_criterion
        else:
            criterion = initialize_gan_criterion(section)
        return cls(criterion=criterion, **params_epoch)

    def _adversarial(self, netD, real_Y, fake_Y):
        """(1) discriminator step and the generator's adversarial term, from one forward of ``netD``"""
        return AdversarialScores(self.criterion.losses["adversarial"], self.criterion.weights["adversarial"], netD, real_Y, fake_Y)

    def step_losses(self, networks, batch_images, batch_targets, patch_ids=None):
        raise NotImplementedError("Attempted to evaluate abstract GAN. Choose different GAN epoch iteration.")


class GanImagePool:
    """the reference's image buffer as far as an evaluation meets it: a fresh pool returns its input"""

    def __init__(self, pool_size):
        self.pool_size = pool_size

    def query(self, images):
        return images


class SupervisedCycleGanEpoch(SupervisedGanEpoch):
    """CycleGAN (gan_epochs.py:61-140): networks ``generator_X``, ``generator_Y``, ``discriminator_X``, ``discriminator_Y``; criterion a ``cycle_loss``
    whose generator members are multihead losses with an ``adversarial`` (mse against the target tensor) and a ``cycle`` (l1) head.  ``netD_X`` is scored
    on ``real_Y`` / ``fake_Y`` as the reference does.  Each discriminator runs once, as ``netD.model.forward_multi(cat[real, fake])``: the reference's
    generator step reaches the same discriminator as ``netD.forward(fake)`` (gan_epochs.py:122), which equals the shared run only for a discriminator without
    runtime wrappers -- the scenario's case (train_cyclegan.yml).  ``pool_size`` is accepted and unused: nothing is stored between evaluations."""

    def __init__(self, criterion, pool_size=0):
        super().__init__(criterion)
        self.fake_X_pool = GanImagePool(pool_size)
        self.fake_Y_pool = GanImagePool(pool_size)

    def step_losses(self, networks, batch_images, batch_targets, patch_ids=None):
        netG_X, netG_Y = networks["generator_X"], networks["generator_Y"]
        netD_X, netD_Y = networks["discriminator_X"], networks["discriminator_Y"]
        crit = self.criterion
        with torch.no_grad():
            real_X, real_Y = batch_images, batch_targets
            fake_Y = call_network(netG_X, real_X)
            rec_X = call_network(netG_Y, fake_Y)
            fake_X = call_network(netG_Y, real_Y)
            rec_Y = call_network(netG_X, fake_X)
            adv_X = AdversarialScores(crit.loss_D_X, 1.0, netD_X, real_Y, self.fake_X_pool.query(fake_Y), multi=True)
            adv_Y = AdversarialScores(crit.loss_D_Y, 1.0, netD_Y, real_X, self.fake_Y_pool.query(fake_X), multi=True)
            target = float(adversarial.DiscriminatorLoss.get_target(True))
            sides = (("netG_X", crit.loss_G_X, {"adversarial": (adv_X.pred_fake, target), "cycle": (rec_X, real_X)}),
                     ("netG_Y", crit.loss_G_Y, {"adversarial": (adv_Y.pred_fake, target), "cycle": (rec_Y, real_Y)}))
            terms = []
            for name, loss_G, heads in sides:
                assert loss_G.losses.keys() == heads.keys(), str(loss_G.losses.keys()) + "!=" + str(heads.keys())
                terms += [map_term(loss_G, key, *heads[key]) for key in loss_G.losses]
            means = compound.map_losses(terms).per_pair
            generator, at = [], 0
            for name, loss_G, heads in sides:
                partial = [(key, means[at + i] * terms[at + i].weight) for i, key in enumerate(loss_G.losses)]
                at += len(partial)
                total = partial[0][1]
                for _, value in partial[1:]:
                    total = total + value
                generator.append((name, total, partial))
            total = generator[0][1] + generator[1][1] + adv_X.discriminator + adv_Y.discriminator
            losses = StepLosses([("total", total)])
            for name, side_total, partial in generator:
                losses[name + "_total"] = side_total
                for key, value in partial:
                    losses["%s_%s" % (name, key)] = value
            losses["netD_X_total"] = adv_X.discriminator
            losses["netD_Y_total"] = adv_Y.discriminator
            dbg_data = {"real_X": real_X[-1], "fake_Y": fake_Y[-1], "rec_X": rec_X[-1], "real_Y": real_Y[-1], "fake_X": fake_X[-1], "rec_Y": rec_Y[-1]}
        return losses, dbg_data
