"""mirror of mdir/learning/validation.py:11-165: the validation tasks of a scenario's ``validation`` section.

Only validations without a data loader are provided (``data: null``: the criterion is a score of the network, e.g. ``cirdatasetap``);
a ``data`` key that names a loader, and any validation type other than SingleValidation / MultiCriterialValidation, raise
NotImplementedError."""
import copy

from ..components.optim.score import initialize_score


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

    def __init__(self, criterion, network_overlay, frequency, decisive_criterion):
        self.data_loader = None
        self.criterion = criterion
        self.network_overlay = network_overlay
        self.frequency = frequency
        self.decisive_criterion = decisive_criterion

    @classmethod
    def initialize(cls, params_validation, data=None, params_data=None, default_criterion=None, network=None):
        net_defaults = network.network_params.runtime.get("data", {}) if network is not None else {}
        data_key = params_validation.pop("data")
        if data_key is not None:
            raise NotImplementedError("validation data %r: loader-based (loss) validations are not provided by this build; "
                                      "use data: null with a score criterion" % (data_key,))
        criterion_section = params_validation.pop("criterion")
        if criterion_section == "default":
            if default_criterion is None:
                raise ValueError("Criterion cannot be 'default' when default criterion is not specified")
            criterion = default_criterion
        else:
            criterion = initialize_score(copy.deepcopy({**net_defaults, **criterion_section}))
        network_overlay = params_validation.pop("network_overlay")
        frequency = params_validation.pop("frequency")
        assert not params_validation, params_validation.keys()
        return cls(criterion=criterion, network_overlay=network_overlay, frequency=frequency,
                   decisive_criterion=criterion.decisive_criterion)

    def validations(self, epoch):
        return [("val", self)] if self.should_validate(epoch) else []

    def should_validate(self, epoch):
        return epoch is None or bool(self.frequency and (epoch + 1) % self.frequency == 0)

    def validate(self, network, device, logger):
        if self.network_overlay:
            network = network.overlay_params(copy.deepcopy(self.network_overlay), device)
        network.eval()
        return self.criterion(network, device, logger)

    def __repr__(self):
        return "%s (criterion: %s, network_overlay: %s, frequency: %s, decisive_criterion: %s)" % (
            type(self).__name__, self.criterion, self.network_overlay, self.frequency, self.decisive_criterion)


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
