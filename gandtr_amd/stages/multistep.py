"""``infer_and_learn_whitening`` stage -- mdir/stages/multistep.py:8-43 (template mdir/examples/iccv23/parameters/whitening.yml): describe the
images a whitening dataset lists and learn the whitening that the ``cirwhiten`` wrapper of the evaluation loads.  The dataset pkl holds ``cids``
(image identifiers), ``qidxs`` and ``pidxs`` (positions of matching query / positive pairs).  Decoding, descriptors and the learner run on the
device and the descriptors stay there in between.  Not mirrored: a ``dataset_pkl`` or ``network.path`` that is a URL (download plumbing is the
scenario's download step; pass a local file)."""
import os
import pickle

from ..tools import utils
from . import whiten
from .infer import embed_files


def _is_url(value):
    return isinstance(value, str) and "://" in value and not value.startswith("file://")


def infer_and_learn_whitening(params, data):
    """Perform inference and learn whitening on resulting descriptors.  ``params["whitening"]`` has exactly the keys ``type`` (``lw`` / ``pca``),
    ``dataset_pkl`` and ``directory``; with a directory the result is stored as ``<directory>/whitening/<type>-<pkl name up to its first "-">.pkl``
    (a ``{"m", "P"}`` pickle) and an existing file skips the stage.  The rest of ``params`` is what ``infer`` takes on its file route.  ``pca``
    hands the learner the descriptors alone (the reference passes the four ``lw`` columns to either learner, which ``learn_pca_whitening`` cannot
    unpack)."""
    assert not data
    whitening = params.pop("whitening")
    assert whitening.keys() == {"type", "dataset_pkl", "directory"}

    # Handle saving and potential execution skipping
    path = None
    if whitening["directory"]:
        path = os.path.join(whitening["directory"], "whitening",
                            "%s-%s.pkl" % (whitening["type"], whitening["dataset_pkl"].rsplit("/", 1)[-1].split("-", 1)[0]))
        if os.path.exists(path):
            return {"status": "skipped", "whitening_path": path}, None
    for what, value in (("whitening.dataset_pkl", whitening["dataset_pkl"]), ("network.path", (params.get("network") or {}).get("path"))):
        if _is_url(value):
            raise NotImplementedError("infer_and_learn_whitening: %s = %s is a URL; downloads are not mirrored here, pass a local file" % (what, value))
    learn_whitening = {"lw": whiten.learn_lw_whitening, "pca": whiten.learn_pca_whitening}[whitening["type"]]
    if path:
        os.makedirs(os.path.dirname(path), exist_ok=True)

    pkl = utils.fs_load_pickle(whitening["dataset_pkl"])

    # Infer: D x N on the device; the learners take N x D
    paths = ["/".join([x[-2:], x[-4:-2], x[-6:-4], x]) for x in pkl["cids"]]
    metadata_infer, vecs = embed_files(params, paths)
    descriptors = vecs.t().contiguous()

    # Learn whitening
    if whitening["type"] == "pca":
        metadata_learn_whitening, whit = learn_whitening({}, (descriptors,))
    else:
        qidxs, pidxs = [pkl["cids"][x] for x in pkl["qidxs"]], [pkl["cids"][x] for x in pkl["pidxs"]]
        metadata_learn_whitening, whit = learn_whitening({}, (pkl["cids"], descriptors, qidxs, pidxs))

    # Store
    if path:
        with open(path, "wb") as handle:
            pickle.dump(whit, handle)

    return {"infer": metadata_infer, "learn_whitening": metadata_learn_whitening, "whitening_path": path}, whit
