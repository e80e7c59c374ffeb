"""CUT's contrastive head on the host (no GPU): the registries, PatchSampleF's module tree, the CPU path against the fixture the reference wrote
(tests/golden/make_patchnce_golden.py) -- pooled rows, the ids a seed draws, row losses, layer means and totals for both ``batch_dim_for_bmm`` values,
``use_mlp=False``; in float64 to 1e-6 and in fp32 within the fp32 bound --, the whole ``calculate_nce_loss`` forward, and the refused configurations."""
import numpy as np
import pytest
import torch

from patchnce_fixture import GOLD, N_HEAD, N_PIPE, NCE_LAYERS, PIPE_PATCHES, TEMPERATURE, WEIGHT, criterion, head_case, pipe_case

# train_cut.yml:21-30, the featdown block, and :74-80, the nce criterion
CUT_FEATDOWN = {"architecture": "official_p2p_mlp", "input_nc": 3, "nc": 256, "nce_layers": "4,8,12,16"}
CUT_NCE = {"loss": "multilayer_patchnce_loss", "batch_dim_for_bmm": 1, "nce_layers": "4,8,12,16", "num_patches": 256, "temperature": 0.07, "weight": 1}


def test_registry_labels_and_mdir_shim():
    from gandtr_amd.components.model import network as registry
    from gandtr_amd.components.model.network import p2p_networks
    from gandtr_amd.components.optim import criterion as crit_registry
    from gandtr_amd.components.optim.criterion import patchnce
    assert registry.MODEL_LABELS["official_p2p_mlp"] is p2p_networks.PatchSampleF
    import mdir.components.model.network as ref_registry
    import mdir.components.optim.criterion.patchnce as shim
    assert ref_registry.MODEL_LABELS["official_p2p_mlp"] is p2p_networks.PatchSampleF
    assert shim is patchnce
    assert set(crit_registry.CRITERIA) == {"contrastive", "triplet"}
    with pytest.raises(NotImplementedError):
        crit_registry.initialize_criterion(dict(CUT_NCE))
    crit = patchnce.initialize_patchnce_criterion(dict(CUT_NCE))
    assert isinstance(crit, patchnce.MultilayerPatchNCELoss)
    assert crit.nce_layers == [4, 8, 12, 16] and crit.num_patches == 256 and len(crit.losses) == 4
    assert all(isinstance(l, patchnce.PatchNCELoss) and l.batch_dim_for_bmm == 1 and l.temperature == 0.07 for l in crit.losses)
    assert set(patchnce.PATCHNCE_CRITERIA) == {"multilayer_patchnce_loss"}
    assert patchnce.initialize_patchnce_criterion(None) is None
    with pytest.raises(NotImplementedError):
        patchnce.initialize_patchnce_criterion({"loss": "discriminator_loss"})


def test_constructor_runs_no_generator_forward_and_needs_no_gpu(monkeypatch):
    from gandtr_amd.components.model import network as registry
    from gandtr_amd.components.model.network import p2p_networks

    def refuse(*a, **k):
        raise AssertionError("the constructor ran a generator")

    monkeypatch.setattr(p2p_networks.ResnetGenerator, "__init__", refuse)
    monkeypatch.setattr(torch.nn.Module, "cuda", refuse)
    netF = registry.initialize_model(dict(CUT_FEATDOWN))
    assert netF.meta == {"in_channels": 3, "out_channels": 256} and netF.mlp_init and netF.use_mlp and netF.nc == 256
    assert [getattr(netF, "mlp_%d" % i)[0].in_features for i in range(4)] == [128, 256, 256, 256]
    assert all(p.device.type == "cpu" for p in netF.parameters())
    # any tap the generator has: stem 64, the two down convs 128 / 256, the blocks 256, the up convs 128 / 64, the head 3
    assert p2p_networks.generator_tap_channels([1, 3, 4, 6, 7, 9, 10, 18, 19, 21, 22, 24, 26, 27]) == [64, 64, 128, 128, 256, 256, 256, 256, 128, 128, 64, 64, 3, 3]
    assert p2p_networks.generator_tap_channels([2, 5, 8], ngf=16, n_blocks=2) == [16, 32, 64]


def test_state_dict_keys_and_shapes_are_the_references():
    for i in range(N_HEAD):
        netF, _, _, shape, p = head_case(i)
        if not shape[5]:
            assert list(netF.state_dict()) == []
            continue
        sd = netF.state_dict()
        assert list(sd) == [str(k) for k in GOLD[p + "keys"]]
        assert [list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()] == GOLD[p + "shapes"].tolist()
    from gandtr_amd.components.model.network import p2p_networks
    full = p2p_networks.PatchSampleF(**{k: v for k, v in CUT_FEATDOWN.items() if k != "architecture"})
    assert list(full.state_dict()) == ["mlp_%d.%d.%s" % (i, j, n) for i in range(4) for j in (0, 2) for n in ("weight", "bias")]


def _cpu_head(i, dtype):
    """head case i through the mirror's CPU path in ``dtype``: (pooled q, pooled k, ids of both calls, shape, fixture prefix)"""
    netF, qmap, kmap, shape, p = head_case(i)
    netF = netF.to(dtype)
    np.random.seed(80 + i)
    with torch.no_grad():
        k_pool, ids = netF([kmap.to(dtype)], num_patches=shape[4], patch_ids=None)
        q_pool, ids_q = netF([qmap.to(dtype)], num_patches=shape[4], patch_ids=ids)
    return q_pool, k_pool, ids, ids_q, shape, p


@pytest.mark.parametrize("i", range(N_HEAD))
def test_cpu_head_reproduces_the_fixture(i):
    """The fixture's head cases are the reference's modules run in float64 (an fp32 run carries up to 6e-6 of its own in a row loss, and which 6e-6 depends
    on the machine's BLAS code path).  The mirror's CPU path run in float64 reproduces them to 1e-6 ABSOLUTE on every machine: pooled rows (stored rounded
    to fp32), the ids drawn under the seed, row losses, partial keys, layer means and totals, for both groups values."""
    q_pool, k_pool, ids, ids_q, (B, C, H, W, P, nc), p = _cpu_head(i, torch.float64)
    assert ids[0].dtype == torch.long and np.array_equal(ids[0].numpy(), GOLD[p + "ids"]) and torch.equal(ids_q[0], ids[0])
    assert ids[0].numel() == min(P, H * W) and k_pool[0].shape == (B * min(P, H * W), nc or C)
    assert float((k_pool[0] - torch.from_numpy(GOLD[p + "k"]).double()).abs().max()) <= 1e-6
    assert float((q_pool[0] - torch.from_numpy(GOLD[p + "q"]).double()).abs().max()) <= 1e-6
    for groups in (1, B):
        g = p + "g%d_" % groups
        crit = criterion(groups, "0", P)
        with torch.no_grad():
            out = crit(q_pool, k_pool)
        assert list(out.partial) == [str(k) for k in GOLD[g + "keys"]] == ["layer0"]
        assert float((crit.row_losses[0] - torch.from_numpy(GOLD[g + "rows0"])).abs().max()) <= 1e-6
        assert abs(float(out.partial["layer0"]) - float(GOLD[g + "means"][0])) <= 1e-6
        assert abs(float(out.total) - float(GOLD[g + "total"])) <= 1e-6
        assert out.total.dim() == 0


@pytest.mark.parametrize("i", range(N_HEAD))
def test_cpu_head_in_fp32_is_within_the_fp32_bound_of_the_fixture(i):
    """The same path in fp32, as it is used.  Pooled rows (unit rows, a few 2^-24 of error per element) within 1e-6.  Row losses within the fp32 bound of
    the exact value, u = 2^-24: 2 (d + 2) u / T + (n + 16) u + 16 u |loss| for the dot products, exp, sum and log (unit rows), plus what rows that moved
    by at most 1e-6 per element move the logits: |dq|_2, |dk|_2 <= 1e-6 sqrt(d), a logit moves by at most (|dq|_2 + |dk|_2) / T, the loss by twice that."""
    q_pool, k_pool, ids, _, (B, C, H, W, P, nc), p = _cpu_head(i, torch.float32)
    assert q_pool[0].dtype == torch.float32 and np.array_equal(ids[0].numpy(), GOLD[p + "ids"])
    assert float((k_pool[0] - torch.from_numpy(GOLD[p + "k"])).abs().max()) <= 1e-6
    assert float((q_pool[0] - torch.from_numpy(GOLD[p + "q"])).abs().max()) <= 1e-6
    d, u = q_pool[0].shape[1], 2.0 ** -24
    for groups in (1, B):
        g = p + "g%d_" % groups
        crit = criterion(groups, "0", P)
        with torch.no_grad():
            out = crit(q_pool, k_pool)
        want = torch.from_numpy(GOLD[g + "rows0"])
        n = want.numel() // groups
        tol = 2 * (d + 2) * u / TEMPERATURE + (n + 16) * u + 16 * u * want.abs() + 4 * 1e-6 * d ** 0.5 / TEMPERATURE
        assert crit.row_losses[0].dtype == torch.float32 and bool(((crit.row_losses[0].double() - want).abs() <= tol).all())
        assert out.total.dtype == torch.float32 and out.total.dim() == 0 and list(out.partial) == ["layer0"]
        assert abs(float(out.partial["layer0"]) - float(GOLD[g + "means"][0])) <= float(tol.mean()) + 4 * u * abs(float(GOLD[g + "means"][0]))
        assert abs(float(out.total) - float(GOLD[g + "total"])) <= float(tol.mean()) + 4 * u * abs(float(GOLD[g + "total"]))


@pytest.mark.parametrize("i", range(N_PIPE))
def test_cpu_calculate_nce_loss_reproduces_the_fixture(i):
    """the whole forward of calculate_nce_loss: the seed draws the reference's ids (returned per layer), rows and totals within 1e-5 relative (two generator
    passes of 24 convs in fp32 on another thread count than the fixture's)"""
    from gandtr_amd.components.optim.criterion import patchnce
    netG, netF, src, tgt, ids, p = pipe_case(i)
    B = src.shape[0]
    for groups in sorted({1, B}):
        g = p + "g%d_" % groups
        crit = criterion(groups)
        np.random.seed(95 + i)
        with torch.no_grad():
            out = patchnce.calculate_nce_loss(crit, netG, netF, src, tgt)
        assert list(out.partial) == [str(k) for k in GOLD[g + "keys"]] == ["layer4", "layer8", "layer12", "layer16"]
        for l in range(4):
            want = torch.from_numpy(GOLD[g + "rows%d" % l])
            assert crit.row_losses[l].shape == want.shape
            assert float(((crit.row_losses[l] - want).abs() / (1 + want.abs())).max()) <= 1e-5
        assert float(out.total) == pytest.approx(float(GOLD[g + "total"]), rel=1e-5)
        np.testing.assert_allclose([float(v) for v in out.partial.values()], GOLD[g + "means"], rtol=1e-5)
    # the stored ids give the same result as the seed
    with torch.no_grad():
        again = patchnce.calculate_nce_loss(crit, netG, netF, src, tgt, patch_ids=ids)
    assert float(again.total) == float(out.total)


def test_rejected_configurations():
    from gandtr_amd.components.model.network import p2p_networks
    from gandtr_amd.components.optim.criterion import patchnce
    with pytest.raises(NotImplementedError, match="reflection-padded"):
        p2p_networks.PatchSampleF()                                    # the reference's default nce_layers start at layer 0
    with pytest.raises(NotImplementedError, match="reflection-padded"):
        p2p_networks.PatchSampleF(nce_layers="4,25")
    with pytest.raises(ValueError):
        p2p_networks.PatchSampleF(nce_layers="4,99")
    crit = patchnce.PatchNCELoss(batch_dim_for_bmm=3)
    with pytest.raises(ValueError):
        crit(torch.zeros(8, 4), torch.zeros(8, 4))                     # 8 rows do not split into 3 groups
    with pytest.raises(ValueError):
        crit(torch.zeros(9, 4), torch.zeros(9, 5))
    with pytest.raises(ValueError):
        patchnce.MultilayerPatchNCELoss(1, "", 64, 0.07, 1.0)
    # lazily created MLPs land on the features' device, here the CPU
    lazy = p2p_networks.PatchSampleF(input_nc=None, nce_layers=None, nc=8)
    assert not lazy.mlp_init
    with torch.no_grad():
        feats, ids = lazy([torch.randn(2, 5, 4, 4)], num_patches=3)
    assert lazy.mlp_init and lazy.mlp_0[0].in_features == 5 and lazy.mlp_0[0].weight.device.type == "cpu"
    assert feats[0].shape == (6, 8) and ids[0].shape == (3,)
    with torch.no_grad():
        whole, none = lazy([torch.randn(2, 5, 4, 4)], num_patches=0)
    assert whole[0].shape == (2, 8, 4, 4) and none == [[]]
