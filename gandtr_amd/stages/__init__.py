"""Stage (operator) layer: ``stage(params: dict, data: tuple) -> (metadata: dict, *output_columns)``
(contract: mdir/examples/perform_scenario.py:129).  ``infer`` and ``validate`` (descriptor extraction + ranking, the retrieval
evaluation's caller of the path) are on the hot path's boundary; the whitening stages (``whiten``, ``learn_lw_whitening``,
``learn_pca_whitening``, ``paste_pca_normalize``, ``l2_normalize``) and ``infer_and_learn_whitening`` belong to the "next" rows of
SURVEY.md section 8f."""
from . import infer as _infer_module
from .infer import infer
from .validate import rank_images, validate
from .multistep import infer_and_learn_whitening
from .whiten import l2_normalize, learn_lw_whitening, learn_pca_whitening, paste_pca_normalize, whiten

FUNCTIONS = {"mdir.stages.infer.infer": infer, "mdir.stages.validate.validate": validate, "mdir.stages.whiten.whiten": whiten,
             "mdir.stages.whiten.learn_lw_whitening": learn_lw_whitening, "mdir.stages.whiten.learn_pca_whitening": learn_pca_whitening,
             "mdir.stages.whiten.paste_pca_normalize": paste_pca_normalize, "mdir.stages.whiten.l2_normalize": l2_normalize,
             "mdir.stages.multistep.infer_and_learn_whitening": infer_and_learn_whitening,
             # this build's own stage (no reference counterpart): the validate arithmetic with ranks / scores as output columns
             "gandtr_amd.stages.validate.rank_images": rank_images}
