"""mirror of mdir/components/optim/score/__init__.py: ``initialize_score`` builds a validation score from its parameters.
Only ``cirdatasetap`` (retrieval mAP on a cirtorch test dataset) is provided; ``visual`` raises NotImplementedError."""
from . import cirscore

SCORES = {
    "cirdatasetap": cirscore.CirDatasetAp,
}


def initialize_score(params):
    kind = params.pop("type")
    if kind not in SCORES:
        raise NotImplementedError("score type %r is not provided by this build (available: %s)" % (kind, ", ".join(sorted(SCORES))))
    return SCORES[kind](params)
