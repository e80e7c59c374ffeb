"""PCA whitening stages without a device: the eigh restatement (tests/pca_whiten_ref.py) against the reference's golden vectors
(tests/golden/pca_whiten.npz), the stage signatures' device-free branches, the registries, and the bookkeeping of
``infer_and_learn_whitening`` that runs before anything is loaded."""
import os
import pickle

import numpy as np
import pytest
import torch

import pca_whiten_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pca_whiten.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("case", range(len(R.PCA_CASES)))
def test_restatement_reproduces_pcawhitenlearn(gold, case):
    d, n, shrink = R.PCA_CASES[case]
    X = gold["pca_X_%d" % case]
    assert X.dtype == np.float32 and X.shape == (d, n) and np.array_equal(X, R.descriptors(case, d, n).T)
    m, P, eig, shrunk = R.pcawhitenlearn(X.astype(np.float64), shrink)
    assert np.abs(m - gold["pca_m_%d" % case]).max() < 1e-14
    assert np.abs(eig - gold["pca_eig_%d" % case]).max() < 1e-9 * eig[0]
    scale = np.sqrt(shrunk)[:, None]
    assert R.rows_up_to_sign_abs(P * scale, gold["pca_P_%d" % case] * scale) < 1e-8


@pytest.mark.parametrize("case", range(len(R.PASTE_CASES)))
def test_restatement_reproduces_paste_pca_normalize(gold, case):
    d1, d2, n, dims = R.PASTE_CASES[case]
    out = R.paste_pca_normalize(R.paste_inputs(case), dims)
    assert out.shape == (n, d1 + d2)
    ref = gold["paste_out_%d" % case]
    if dims is None:
        out = out[::R.PASTE_STORED_ROWS]
    assert np.abs(out - ref).max() < 1e-10


def test_restatement_reproduces_l2_normalize(gold):
    a, _ = R.paste_inputs(0)
    assert np.abs(R.l2_normalize(3.0 * a.astype(np.float64)) - gold["l2n_out"]).max() < 1e-14


def test_stage_empty_branches_and_unknown_parameters():
    import mdir.stages.whiten as stage
    assert stage.learn_pca_whitening({"shrink": None}, (np.zeros((0, 8)),)) == ({"status": "Empty whitening produced"}, None)
    assert stage.learn_pca_whitening({}, (np.zeros((0,)),)) == ({"status": "Empty whitening produced"}, None)
    empty = np.zeros((0,))
    meta, value = stage.paste_pca_normalize({"dimensions": 4}, (empty, empty))
    assert meta == {} and value is empty
    meta, value = stage.l2_normalize({}, (np.zeros((0, 8)),))
    assert meta == {} and value.shape == (0, 8)
    with pytest.raises(AssertionError):
        stage.learn_pca_whitening({"shrink": 2, "dimensions": 3}, (np.ones((4, 2)),))
    with pytest.raises(AssertionError):
        stage.paste_pca_normalize({"dimensions": None, "shrink": 1}, (np.ones((4, 2)),))
    with pytest.raises(AssertionError):
        stage.l2_normalize({"dimensions": 2}, (np.ones((4, 2)),))
    with pytest.raises(KeyError):
        stage.paste_pca_normalize({}, (np.ones((4, 2)),))                     # `dimensions` is popped without a default (whiten.py:101)
    with pytest.raises(AssertionError):
        stage.paste_pca_normalize({"dimensions": None}, (np.ones((4, 2)), np.ones((5, 2))))     # columns of unequal length


def test_stages_raise_without_a_device(monkeypatch):
    import mdir.stages.whiten as stage
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = R.descriptors(0, 8, 40).astype(np.float64)
    with pytest.raises(RuntimeError, match="HIP device"):
        stage.learn_pca_whitening({}, (x,))
    with pytest.raises(RuntimeError, match="HIP device"):
        stage.paste_pca_normalize({"dimensions": 4}, (x, x))
    with pytest.raises(RuntimeError, match="HIP device"):
        stage.paste_pca_normalize({"dimensions": None}, (x, x))
    with pytest.raises(RuntimeError, match="HIP device"):
        stage.l2_normalize({}, (x,))


def test_host_argument_errors_need_no_device():
    from gandtr_amd import whiten_learn
    with pytest.raises(ValueError):
        whiten_learn.pcawhitenlearn(torch.zeros(8, 40))                       # a CPU tensor
    with pytest.raises(ValueError):
        whiten_learn.pca_project_normalize(torch.zeros(40, 8, dtype=torch.float64), 4)
    with pytest.raises(ValueError):
        whiten_learn.l2n_rows(torch.zeros(40, 8, dtype=torch.float64))


def test_c_abi_validates_before_any_device_call():
    import ctypes
    from gandtr_amd import _hip
    lib = _hip.load()
    need = ctypes.c_size_t()
    _hip.check(lib.gdt_pca_whiten_learn_workspace_bytes(100, 16, ctypes.byref(need)))
    small = need.value
    _hip.check(lib.gdt_pca_whiten_learn_workspace_bytes(100, 32, ctypes.byref(need)))
    assert need.value > small > 4 * 16 * 16 * 8
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_pca_whiten_learn_workspace_bytes(100, 15, ctypes.byref(need)))         # odd descriptor size
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_pca_whiten_learn_workspace_bytes(100, 8194, ctypes.byref(need)))
    _hip.check(lib.gdt_pca_project_normalize_workspace_bytes(100, 63, ctypes.byref(need)))      # an odd width is padded
    padded = need.value
    _hip.check(lib.gdt_pca_project_normalize_workspace_bytes(100, 64, ctypes.byref(need)))
    assert padded == need.value
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_pca_whiten_learn(None, 100, 16, 17, None, None, None, None, None, 0, None))   # shrink out of 1..d
    with pytest.raises(ValueError):
        _hip.check(lib.gdt_pca_project_normalize(None, 100, 16, 0, None, None, None, 0, None))           # dims out of 1..d


def test_registries():
    import mdir
    import mdir.stages.multistep as multistep
    import mdir.stages.whiten as stage
    from gandtr_amd import stages
    import gandtr_amd.stages.multistep as own
    assert multistep is own and mdir.stages.multistep is own
    assert stages.FUNCTIONS["mdir.stages.whiten.learn_pca_whitening"] is stage.learn_pca_whitening
    assert stages.FUNCTIONS["mdir.stages.whiten.paste_pca_normalize"] is stage.paste_pca_normalize
    assert stages.FUNCTIONS["mdir.stages.whiten.l2_normalize"] is stage.l2_normalize
    assert stages.FUNCTIONS["mdir.stages.multistep.infer_and_learn_whitening"] is multistep.infer_and_learn_whitening
    assert stages.FUNCTIONS["mdir.stages.whiten.learn_lw_whitening"] is stage.learn_lw_whitening     # the earlier entries are still there
    assert stages.FUNCTIONS["mdir.stages.whiten.whiten"] is stage.whiten


def _params(whitening, network_path=None):
    return {"data": {"test": {"dataset": {"image_dir": "ims/*", "image_size": 64, "name": "CirImageList"}}},
            "network": {"path": network_path, "runtime": {"wrappers": "cirmultiscale:True"}},
            "output": {"debug": True, "inference": {"name": "embedding"}}, "whitening": whitening}


def test_infer_and_learn_whitening_bookkeeping(tmp_path):
    from mdir.stages.multistep import infer_and_learn_whitening
    with pytest.raises(AssertionError):
        infer_and_learn_whitening(_params({"type": "lw", "dataset_pkl": "x-whiten.pkl"}), ())                      # a key is missing
    with pytest.raises(AssertionError):
        infer_and_learn_whitening(_params({"type": "lw", "dataset_pkl": "x-whiten.pkl", "directory": None, "shrink": 1}), ())
    with pytest.raises(AssertionError):
        infer_and_learn_whitening(_params({"type": "lw", "dataset_pkl": "x-whiten.pkl", "directory": None}), (["a"],))   # takes no data
    # an existing target skips the stage before the pkl (which does not exist) or the network is touched
    target = tmp_path / "whitening" / "lw-retrieval.pkl"
    target.parent.mkdir()
    with open(target, "wb") as handle:
        pickle.dump({"m": np.zeros((2, 1)), "P": np.eye(2)}, handle)
    whitening = {"type": "lw", "dataset_pkl": str(tmp_path / "dbs" / "retrieval-SfM-120k-whiten.pkl"), "directory": str(tmp_path)}
    assert infer_and_learn_whitening(_params(whitening), ()) == ({"status": "skipped", "whitening_path": str(target)}, None)
    # the other type has its own file: not skipped, and a missing pkl is reported as such
    with pytest.raises(FileNotFoundError):
        infer_and_learn_whitening(_params(dict(whitening, type="pca")), ())
    with pytest.raises(KeyError):
        infer_and_learn_whitening(_params(dict(whitening, type="zca")), ())


def test_infer_file_route_with_nothing_to_do():
    from mdir.stages.infer import infer
    params = _params(None)
    del params["whitening"]
    assert infer(params, ([],)) == ({"status": "skipped"}, [], [])
    assert infer({"output": {"inference": {"name": "embedding"}}}, ([],)) == ({"status": "skipped"},)       # the in-memory route as before


def test_infer_and_learn_whitening_refuses_urls(tmp_path):
    from mdir.stages.multistep import infer_and_learn_whitening
    url = "http://cmp.felk.cvut.cz/cnnimageretrieval/data/train/dbs/retrieval-SfM-120k-whiten.pkl"      # the template's value (whitening.yml:16)
    with pytest.raises(NotImplementedError, match="local file"):
        infer_and_learn_whitening(_params({"type": "lw", "dataset_pkl": url, "directory": None}), ())
    with pytest.raises(NotImplementedError, match="local file"):
        infer_and_learn_whitening(_params({"type": "lw", "dataset_pkl": url, "directory": str(tmp_path)}), ())
    assert not (tmp_path / "whitening").exists()
    local = tmp_path / "retrieval-whiten.pkl"
    with open(local, "wb") as handle:
        pickle.dump({"cids": [], "qidxs": [], "pidxs": []}, handle)
    with pytest.raises(NotImplementedError, match="network.path"):
        infer_and_learn_whitening(_params({"type": "pca", "dataset_pkl": str(local), "directory": None}, "https://example.org/net.pth"), ())
