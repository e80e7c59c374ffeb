"""PCA whitening on the GPU (second half of gandtr_amd/csrc/whiten_learn.hip through the C ABI): ``pcawhitenlearn``, the projection of
``paste_pca_normalize``, ``l2_normalize``, their stages, the file route of ``infer`` and ``infer_and_learn_whitening``.  Against the reference's
golden vectors (tests/golden/pca_whiten.npz), the eigh restatement (tests/pca_whiten_ref.py) and sign-free identities.  float64 throughout; rows of
P are compared up to sign.  Every check prints its measured figure before it asserts (pytest -s shows them)."""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

import pca_whiten_ref as R
from gandtr_amd import whiten_learn
from gandtr_amd.tools import synth
from oracle import whiten_oracle as W

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pca_whiten.npz")
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _figure(name, value, gate):
    print("%s: %.3e (gate %.0e, margin %.3g)" % (name, value, gate, value / gate))
    return value


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ------------------------------------------------------------------------------------------------------------ 1. fixture cases
@pytest.mark.parametrize("case", range(len(R.PCA_CASES)))
def test_pcawhitenlearn_golden_vectors_from_the_reference(cuda_device, gold, case):
    d, n, shrink = R.PCA_CASES[case]
    X = torch.from_numpy(gold["pca_X_%d" % case]).to(cuda_device)
    m, P, info = whiten_learn.pcawhitenlearn(X, shrink, return_info=True)
    assert m.shape == gold["pca_m_%d" % case].shape == (d, 1) and P.dtype == torch.float64 and P.shape == (d, d)
    assert _figure("golden %d m" % case, np.abs(m.cpu().numpy() - gold["pca_m_%d" % case]).max(), 1e-14) < 1e-14
    w, w_ref = info["eigenvalues"].cpu().numpy(), gold["pca_eig_%d" % case]
    assert _figure("golden %d eigenvalues / l0" % case, np.abs(w - w_ref).max() / w_ref[0], 1e-9) < 1e-9
    assert _figure("golden %d P rows up to sign" % case, W.rows_up_to_sign(P.cpu().numpy(), gold["pca_P_%d" % case]), 1e-8) < 1e-8


# ------------------------------------------------------------------------------------------------------------ 2. against the restatement
@pytest.mark.parametrize("d,n,shrink", [(64, 1000, None), (130, 700, 20)])
def test_pcawhitenlearn_matches_restatement_up_to_sign(cuda_device, d, n, shrink):
    X = R.descriptors(d, d, n).T.copy()                                                      # D x N float32
    m_ref, P_ref, w_ref, shrunk = R.pcawhitenlearn(X.astype(np.float64), shrink)
    m, P, info = whiten_learn.pcawhitenlearn(torch.from_numpy(X).to(cuda_device), shrink, return_info=True)
    P = P.cpu().numpy()
    assert np.abs(m.cpu().numpy() - m_ref).max() < 1e-14
    assert _figure("restatement d=%d eigenvalues / l0" % d, np.abs(info["eigenvalues"].cpu().numpy() - w_ref).max() / w_ref[0], 1e-9) < 1e-9
    scale = np.sqrt(shrunk)[:, None]
    assert _figure("restatement d=%d unit rows" % d, R.rows_up_to_sign_abs(P * scale, P_ref * scale), 1e-7) < 1e-7
    assert _figure("restatement d=%d P rows / row norm" % d, W.rows_up_to_sign(P, P_ref), 1e-7) < 1e-7
    assert info["one_sided"] and 1 <= info["jacobi_sweeps"] <= 30


# ------------------------------------------------------------------------------------------------------------ 3. sign-free identity
@pytest.mark.parametrize("d,n,shrink", [(512, 6000, None), (2048, 12000, None), (512, 6000, 64)])
def test_whitening_identity_at_descriptor_sizes(cuda_device, d, n, shrink):
    """P C P^T = diag(l / l') (the identity without shrinkage), checked on the device in float64; the data of
    test_hip_whiten_learn.py: test_identities_at_full_descriptor_size_2048 (diagonal scaling: condition number below 100)"""
    g = torch.Generator(device=cuda_device).manual_seed(0)
    X = torch.nn.functional.normalize(torch.randn(n, d, generator=g, device=cuda_device) * torch.linspace(1.5, 0.2, d, device=cuda_device)[None, :], dim=1)
    m, P, info = whiten_learn.pcawhitenlearn(X.t(), shrink, return_info=True)
    assert info["one_sided"]
    w = info["eigenvalues"]
    assert bool((w[1:] <= w[:-1]).all()) and float(w[0] / w[-1]) < 100
    Xc = X.double() - m.t()
    C = Xc.t() @ Xc / n
    b = float(w[shrink - 1]) if shrink else 0.0
    target = torch.diag(w / ((1 - b) * w + b)) if shrink else torch.eye(d, device=cuda_device, dtype=torch.float64)
    assert _figure("identity d=%d shrink=%s" % (d, shrink), float((P @ C @ P.t() - target).abs().max()), 1e-8) < 1e-8
    m2, P2 = whiten_learn.pcawhitenlearn(X.t(), shrink)
    assert torch.equal(P2, P) and torch.equal(m2, m)                                        # fixed summation orders: identical bits


# ------------------------------------------------------------------------------------------------------------ 4. singular input
def test_singular_covariance_is_refused_without_shrink(cuda_device):
    X = torch.zeros(8, 40)
    X[:4] = torch.randn(4, 40, generator=torch.Generator().manual_seed(0))                 # rank 4 in d = 8
    with pytest.raises(np.linalg.LinAlgError, match="shrink") as err:
        whiten_learn.pcawhitenlearn(X.to(cuda_device))
    assert "eigenvalue 4 of 8" in str(err.value)                                            # the first of the four (numerically) zero ones
    m, P, info = whiten_learn.pcawhitenlearn(X.to(cuda_device), 2, return_info=True)
    assert bool(torch.isfinite(P).all()) and not info["one_sided"]                           # Cholesky fails: the two-sided form
    w = info["eigenvalues"].cpu().numpy()
    Xd = X.double().numpy()
    C = (Xd - m.cpu().numpy()) @ (Xd - m.cpu().numpy()).T / 40
    assert np.abs(w - np.linalg.eigvalsh(C)[::-1]).max() < 1e-12 * w[0]
    target = np.diag(w / ((1 - w[1]) * w + w[1]))
    Pn = P.cpu().numpy()
    assert _figure("singular P C P^T", np.abs(Pn @ C @ Pn.T - target).max(), 1e-8) < 1e-8


# ------------------------------------------------------------------------------------------------------------ 5. argument errors
def test_argument_errors(cuda_device):
    with pytest.raises(ValueError):
        whiten_learn.pcawhitenlearn(torch.rand(7, 40).to(cuda_device))                      # odd descriptor size
    for shrink in (9, -1):
        with pytest.raises(ValueError):
            whiten_learn.pcawhitenlearn(torch.rand(8, 40).to(cuda_device), shrink)
    with pytest.raises(ValueError):
        whiten_learn.pcawhitenlearn(torch.rand(8, 40))                                      # a CPU tensor
    v = torch.rand(40, 9, dtype=torch.float64)
    with pytest.raises(ValueError):
        whiten_learn.pca_project_normalize(v, 4)
    for dims in (0, 10):
        with pytest.raises(ValueError):
            whiten_learn.pca_project_normalize(v.to(cuda_device), dims)


# ------------------------------------------------------------------------------------------------------------ 6. pca_project_normalize
@pytest.mark.parametrize("case", [0, 1])
def test_pca_project_normalize_golden(cuda_device, gold, case):
    d1, d2, n, dims = R.PASTE_CASES[case]
    a, b = R.paste_inputs(case)
    v = torch.from_numpy(np.concatenate([a, b], axis=1)).to(cuda_device).double()
    out, info = whiten_learn.pca_project_normalize(v, dims, return_info=True)
    assert out.shape == (n, d1 + d2) and out.dtype == torch.float64
    assert info["one_sided"] == ((d1 + d2) % 2 == 0)                                         # an odd width is padded: singular, two-sided
    out = out.cpu().numpy()
    assert _figure("paste %d" % case, np.abs(out - gold["paste_out_%d" % case]).max(), 1e-10) < 1e-10
    assert _figure("paste %d unit rows" % case, np.abs(np.linalg.norm(out, axis=1) - 1).max(), 1e-14) < 1e-14


def test_pca_project_normalize_full_and_rank_deficient(cuda_device):
    a, b = R.paste_inputs(1)                                                                 # 32 + 31 columns
    v = np.concatenate([a, b], axis=1).astype(np.float64)
    out = whiten_learn.pca_project_normalize(torch.from_numpy(v).to(cuda_device), v.shape[1]).cpu().numpy()
    centred = v - v.mean()
    assert _figure("dims = d", np.abs(out - centred / np.linalg.norm(centred, axis=1, keepdims=True)).max(), 1e-12) < 1e-12
    twice = np.concatenate([a, a], axis=1).astype(np.float64)                                # rank 32 in 64 columns: the Gram matrix is singular
    out, info = whiten_learn.pca_project_normalize(torch.from_numpy(twice).to(cuda_device), 8, return_info=True)
    assert bool(torch.isfinite(out).all())                  # (either solver: rounding decides whether the Cholesky of this singular matrix breaks down)
    out = out.cpu().numpy()
    # relative eigengap at 8: 5.9e-2, so the projector is determined to 64 * 2^-52 / 5.9e-2 = 2.4e-13
    assert np.abs(out - R.paste_pca_normalize((a, a), 8)).max() < 1e-10 and np.abs(np.linalg.norm(out, axis=1) - 1).max() < 1e-14


# ------------------------------------------------------------------------------------------------------------ 7. stages
def test_stage_learn_pca_whitening_then_whiten(cuda_device):
    import mdir.stages.whiten as stage
    values = R.descriptors(3, 64, 800)                                                       # N x D, as the stage receives them
    meta, pca = stage.learn_pca_whitening({"shrink": None}, (values,))
    assert set(meta) == {"timings"} and "whitening_learn" in meta["timings"]
    assert pca["m"].shape == (64, 1) and pca["P"].shape == (64, 64) and pca["P"].dtype == np.float64 and pca["m"].dtype == np.float64
    _, P_ref, _, shrunk = R.pcawhitenlearn(values.astype(np.float64).T)
    assert R.rows_up_to_sign_abs(pca["P"] * np.sqrt(shrunk)[:, None], P_ref * np.sqrt(shrunk)[:, None]) < 1e-7
    names = ["im%d" % i for i in range(len(values))]
    meta, names2, out = stage.whiten({"dimensions": 32}, (pca, names, values))
    ref = pca["P"][:32] @ (values.astype(np.float64).T - pca["m"])                           # whitenapply, cirtorch/utils/whiten.py:4-12
    ref = (ref / (np.linalg.norm(ref, axis=0, keepdims=True) + 1e-6)).T
    assert names2 == names and out.dtype == np.float64
    assert _figure("learn_pca_whitening -> whiten", np.abs(out - ref).max(), 1e-12) < 1e-12


def test_stages_paste_and_l2_normalize_through_the_registry(cuda_device, gold):
    from gandtr_amd.stages import FUNCTIONS
    paste, l2n = FUNCTIONS["mdir.stages.whiten.paste_pca_normalize"], FUNCTIONS["mdir.stages.whiten.l2_normalize"]
    for case, (d1, d2, n, dims) in enumerate(R.PASTE_CASES):
        a, b = R.paste_inputs(case)
        meta, value = paste({"dimensions": dims}, (a.astype(np.float64), b.astype(np.float64)))
        assert isinstance(value, np.ndarray) and value.dtype == np.float64 and value.shape == (n, d1 + d2)
        assert (set(meta) == {"timings"} and "pca_compute" in meta["timings"]) if dims else meta == {}
        ref = gold["paste_out_%d" % case]
        assert np.abs((value if dims else value[::R.PASTE_STORED_ROWS]) - ref).max() < 1e-10
        assert np.abs(np.linalg.norm(value, axis=1) - 1).max() < 1e-14
    a, _ = R.paste_inputs(0)
    meta, value = l2n({}, (3.0 * a.astype(np.float64),))
    assert meta == {} and value.dtype == np.float64 and np.abs(value - gold["l2n_out"]).max() < 1e-14


# ------------------------------------------------------------------------------------------------------------ 8. / 9. from image files
def _runtime(wrappers):
    return {"wrappers": wrappers, "data": {"transforms": "pil2np | totensor | normalize", "mean_std": [MEAN, STD]}}


@pytest.fixture(scope="module")
def vgg_checkpoint(tmp_path_factory):
    import gandtr_amd.learning as L
    emb = {"type": "SingleNetwork",
           "model": {"architecture": "cirnet", "cir_architecture": "vgg16", "local_whitening": False, "pooling": "gem",
                     "pretrained": False, "regional": False, "whitening": False},
           "initialize": False, "path": None, "runtime": _runtime("cirfaketuplebatch")}
    net = L.load_network(copy.deepcopy(emb), "cpu")
    net.model.load_state_dict(synth.vgg16_state(0))
    path = tmp_path_factory.mktemp("net") / "vgg.pth"
    torch.save(net.state_dict()["net"], path)
    return str(path)


def _write_images(root, cids):
    """JPEG files of two sizes laid out as <root>/ims/<x[-2:]>/<x[-4:-2]>/<x[-6:-4]>/<x> (no extension, as retrieval-SfM-120k)"""
    from PIL import Image
    rng = np.random.RandomState(5)
    for i, x in enumerate(cids):
        w, h = (96, 80) if i % 2 else (80, 96)
        yy, xx = np.mgrid[0:h, 0:w]
        arr = np.stack([128 + 90 * np.sin(xx / (3.0 + i + c)) * np.cos(yy / (2.0 + 0.7 * i)) + rng.normal(0, 14, (h, w)) for c in range(3)], -1)
        folder = os.path.join(root, "ims", x[-2:], x[-4:-2], x[-6:-4])
        os.makedirs(folder, exist_ok=True)
        with open(os.path.join(folder, x), "wb") as handle:
            Image.fromarray(np.clip(arr, 0, 255).astype(np.uint8)).save(handle, "JPEG", quality=90, subsampling=i % 3)


def _params(root, checkpoint, wrappers, whitening=None):
    params = {"data": {"test": {"dataset": {"image_dir": os.path.join(root, "ims") + "/*", "image_size": 64, "name": "CirImageList"}}},
              "network": {"path": checkpoint, "runtime": _runtime(wrappers)},
              "output": {"debug": True, "inference": {"name": "embedding"}}}
    if whitening is not None:
        params["whitening"] = whitening
    return params


def _cids(count):
    return ["%02dc1d%04xa%02d" % (i % 3, 977 * i + 11, (7 * i) % 100) for i in range(count)]


def _tree_paths(cids):
    return ["/".join([x[-2:], x[-4:-2], x[-6:-4], x]) for x in cids]


def test_infer_file_route(cuda_device, tmp_path, vgg_checkpoint):
    import gandtr_amd.learning as L
    from gandtr_amd.stages import FUNCTIONS
    from gandtr_amd.stages.validate import extract_vectors_from_files
    cids = _cids(10)
    assert len(set(cids)) == 10 and all(len(x) >= 6 for x in cids)
    _write_images(str(tmp_path), cids)
    names = _tree_paths(cids)
    result = FUNCTIONS["mdir.stages.infer.infer"](_params(str(tmp_path), vgg_checkpoint, "cirmultiscale:True"), (names,))
    assert len(result) == 3
    meta, images, vecs = result
    assert images == names and meta["stats"]["items"] == 10
    assert isinstance(vecs, np.ndarray) and vecs.dtype == np.float64 and vecs.shape == (10, 512)
    net = L.load_network({"path": vgg_checkpoint, "runtime": _runtime("cirmultiscale:True")}, cuda_device).eval()
    files = [os.path.join(str(tmp_path), "ims", x) for x in names]
    direct = extract_vectors_from_files(net, files, 64, (MEAN, STD), cuda_device)
    assert np.array_equal(vecs, direct.t().double().cpu().numpy())
    assert np.abs(np.linalg.norm(vecs, axis=1) - 1).max() < 1e-5 and np.abs(vecs[0] - vecs[1]).max() > 1e-3      # descriptors, and not all the same
    with pytest.raises(FileNotFoundError, match="nosuchimage"):
        FUNCTIONS["mdir.stages.infer.infer"](_params(str(tmp_path), vgg_checkpoint, "cirmultiscale:True"), (names + ["ab/cd/ef/nosuchimage"],))


def test_infer_and_learn_whitening_lw(cuda_device, tmp_path, vgg_checkpoint):
    import mdir.stages.whiten as stage
    from gandtr_amd.components.data.wrapper import CirtorchWhiten
    from gandtr_amd.stages import FUNCTIONS
    run = FUNCTIONS["mdir.stages.multistep.infer_and_learn_whitening"]
    root = str(tmp_path)
    cids = _cids(12)
    _write_images(root, cids)
    db = {"cids": cids, "qidxs": [0, 1, 2, 3, 4, 5, 0, 2], "pidxs": [6, 7, 8, 9, 10, 11, 3, 5]}
    os.makedirs(os.path.join(root, "dbs"))
    pkl = os.path.join(root, "dbs", "retrieval-SfM-120k-whiten.pkl")
    with open(pkl, "wb") as handle:
        pickle.dump(db, handle)
    whitening = {"type": "lw", "dataset_pkl": pkl, "directory": os.path.join(root, "out")}
    meta, whit = run(_params(root, vgg_checkpoint, "cirmultiscale:True", dict(whitening)), ())
    target = os.path.join(root, "out", "whitening", "lw-retrieval.pkl")
    assert set(meta) == {"infer", "learn_whitening", "whitening_path"} and meta["whitening_path"] == target
    assert meta["infer"]["stats"]["items"] == 12 and meta["learn_whitening"]["stats"]["vectors_total"] == 8
    assert whit["m"].shape == (512, 1) and whit["P"].shape == (512, 512) and np.isfinite(whit["P"]).all()
    # the same through the two stages one after the other, the descriptors passing through the host as float64
    _, names, vecs = FUNCTIONS["mdir.stages.infer.infer"](_params(root, vgg_checkpoint, "cirmultiscale:True"), (_tree_paths(cids),))
    _, ref = stage.learn_lw_whitening({}, (cids, vecs, [cids[i] for i in db["qidxs"]], [cids[i] for i in db["pidxs"]]))
    assert np.array_equal(whit["m"], ref["m"]) and np.array_equal(whit["P"], ref["P"])
    with open(target, "rb") as handle:
        stored = pickle.load(handle)
    assert set(stored) == {"m", "P"} and np.array_equal(stored["P"], whit["P"]) and np.array_equal(stored["m"], whit["m"])
    wrapper = CirtorchWhiten(target, 16, cuda_device)                                        # the restricted unpickler of the evaluation's wrapper
    assert wrapper.P.shape == (512, 512) and torch.equal(wrapper.P.cpu(), torch.tensor(whit["P"], dtype=torch.float32))
    again = run(_params(root, vgg_checkpoint, "cirmultiscale:True", dict(whitening)), ())
    assert again == ({"status": "skipped", "whitening_path": target}, None)


def test_infer_and_learn_whitening_pca(cuda_device, tmp_path, vgg_checkpoint):
    from gandtr_amd.stages import FUNCTIONS
    root = str(tmp_path)
    cids = _cids(24)
    _write_images(root, cids)
    pkl = os.path.join(root, "small-whiten.pkl")
    with open(pkl, "wb") as handle:
        pickle.dump({"cids": cids, "qidxs": [0, 1], "pidxs": [2, 3]}, handle)
    # the descriptor size cut to 8 by a cirwhiten wrapper reading a {P, m} file written here: 24 vectors give a non-singular 8 x 8 covariance
    rng = np.random.default_rng(0)
    cut = os.path.join(root, "cut.pkl")
    with open(cut, "wb") as handle:
        pickle.dump({"P": np.linalg.qr(rng.normal(size=(512, 512)))[0], "m": rng.normal(size=(512, 1)) * 0.02}, handle)
    wrappers = {"train": None, "eval": {"0_cirwhiten": {"whitening": cut, "dimensions": 8}}}
    whitening = {"type": "pca", "dataset_pkl": pkl, "directory": root}
    meta, whit = FUNCTIONS["mdir.stages.multistep.infer_and_learn_whitening"](_params(root, vgg_checkpoint, wrappers, whitening), ())
    target = os.path.join(root, "whitening", "pca-small.pkl")
    assert meta["whitening_path"] == target and os.path.exists(target) and set(meta["learn_whitening"]) == {"timings"}
    assert whit["P"].shape == (8, 8) and whit["m"].shape == (8, 1)
    _, _, vecs = FUNCTIONS["mdir.stages.infer.infer"](_params(root, vgg_checkpoint, wrappers), (_tree_paths(cids),))
    assert vecs.shape == (24, 8)
    assert _figure("pca from files: m", np.abs(whit["m"][:, 0] - vecs.mean(axis=0)).max(), 1e-14) < 1e-14
    Xc = vecs.T - whit["m"]
    C = Xc @ Xc.T / 24
    assert _figure("pca from files: P C P^T - I", np.abs(whit["P"] @ C @ whit["P"].T - np.eye(8)).max(), 1e-8) < 1e-8
