"""mirror of mdir/learning/epoch_iteration/__init__.py as far as a checkpoint's objective can be EVALUATED: the GAN scenarios' step classes with
``step_losses`` -- the losses the reference's ``_optimization_step`` logs when every optimizer is a no-op and every network is in ``.eval()``.
``SupervisedEpoch`` (the loader-driven retrieval training loop) is not provided."""
from . import gan_epochs, cut_epochs, edges_epochs
from .gan_epochs import StepLosses                     # noqa: F401

EPOCH_ITERATIONS = {
    "SupervisedCycleGanEpoch": gan_epochs.SupervisedCycleGanEpoch,
    "SupervisedCUTEpoch": cut_epochs.SupervisedCutEpoch,
    "SupervisedHEDGANEpoch": edges_epochs.SupervisedHedGanEpoch,
    "SupervisedHEDNGANEpoch": edges_epochs.SupervisedHedNGanEpoch,
}


def initialize_epoch_iteration(params, **kwargs):
    """``{"type": <label of EPOCH_ITERATIONS>, ..options}`` plus ``criterion=`` -> the step class (``params`` is not changed)"""
    params = dict(params)
    kind = params.pop("type")
    if kind not in EPOCH_ITERATIONS:
        raise NotImplementedError("epoch iteration %r is not provided by this build (available: %s)" % (kind, ", ".join(sorted(EPOCH_ITERATIONS))))
    return EPOCH_ITERATIONS[kind].initialize(params, **kwargs)
