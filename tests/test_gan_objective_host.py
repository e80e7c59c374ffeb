"""The GAN scenarios' criteria and step objectives on the host: registries and aliases, the reference's refusals, the C ABI's argument checks without a
GPU, the CPU path of the criteria against the float64 criterion cases of tests/golden/gan_objective.npz, and ``step_losses`` on CPU modules cast to
float64 against the reference's float64 step values (the same ops; only the order of a few sums differs)."""
import ctypes

import pytest
import torch

import gan_objective_fixture as FX

EPS53, mirror_networks, mirror_epoch, cut_ids = FX.EPS53, FX.mirror_networks, FX.mirror_epoch, FX.cut_ids


def test_registries_and_aliases():
    import mdir                                                                      # noqa: F401
    from gandtr_amd.components.optim import criterion
    from gandtr_amd.components.optim.criterion import adversarial, compound, patchnce
    from gandtr_amd.learning import epoch_iteration
    from gandtr_amd.learning.epoch_iteration import cut_epochs, edges_epochs, gan_epochs
    import mdir.components.optim.criterion.compound as alias_compound
    import mdir.learning.epoch_iteration as alias_epochs
    import mdir.learning.epoch_iteration.cut_epochs as alias_cut
    import mdir.learning.epoch_iteration.edges_epochs as alias_edges
    import mdir.learning.epoch_iteration.gan_epochs as alias_gan
    assert alias_compound is compound and alias_epochs is epoch_iteration
    assert (alias_cut, alias_edges, alias_gan) == (cut_epochs, edges_epochs, gan_epochs)
    assert set(compound.GAN_CRITERIA) == {"l1", "mse", "multihead_loss", "combination_loss", "loss_set", "cycle_loss", "discriminator_loss",
                                          "multilayer_patchnce_loss"}
    assert compound.GAN_CRITERIA["discriminator_loss"] is adversarial.DiscriminatorLoss
    assert compound.GAN_CRITERIA["multilayer_patchnce_loss"] is patchnce.MultilayerPatchNCELoss
    assert epoch_iteration.EPOCH_ITERATIONS == {"SupervisedCycleGanEpoch": gan_epochs.SupervisedCycleGanEpoch, "SupervisedCUTEpoch": cut_epochs.SupervisedCutEpoch,
                                                "SupervisedHEDGANEpoch": edges_epochs.SupervisedHedGanEpoch, "SupervisedHEDNGANEpoch": edges_epochs.SupervisedHedNGanEpoch}
    # the registries that existed before are what they were
    assert set(criterion.CRITERIA) == {"contrastive", "triplet"}
    assert set(adversarial.ADVERSARIAL_CRITERIA) == {"discriminator_loss"} and adversarial.KINDS == {"mse": 0, "bce_with_logits": 1}
    assert set(patchnce.PATCHNCE_CRITERIA) == {"multilayer_patchnce_loss"}
    with pytest.raises(NotImplementedError):
        adversarial.DiscriminatorLoss(criterion={"loss": "l1"})
    with pytest.raises(NotImplementedError, match="SupervisedHEDNGANEpoch"):
        epoch_iteration.initialize_epoch_iteration({"type": "SupervisedEpoch"})
    with pytest.raises(NotImplementedError):
        compound.initialize_gan_criterion({"loss": "bce"})


def test_initialisation_through_the_registries():
    from gandtr_amd.components.optim.criterion import adversarial, compound, patchnce
    from gandtr_amd.learning import epoch_iteration
    params = FX.criterion_params("SupervisedCycleGanEpoch")
    crit = compound.initialize_gan_criterion(params)
    assert params == FX.criterion_params("SupervisedCycleGanEpoch")                 # nothing was popped from the caller's dict
    assert isinstance(crit, compound.CycleLoss) and crit.reduction == "mixed"
    assert isinstance(crit.loss_G_X, compound.MultiheadLoss) and isinstance(crit.loss_D_Y, adversarial.DiscriminatorLoss)
    assert isinstance(crit.loss_G_Y.losses["adversarial"], compound.MSELoss) and isinstance(crit.loss_G_Y.losses["cycle"], compound.L1Loss)
    assert crit.loss_G_X.reduction == "mean" and crit.loss_G_X.weights == {"adversarial": 1, "cycle": 10}
    cut = compound.initialize_gan_criterion(FX.criterion_params("SupervisedCUTEpoch"))
    assert isinstance(cut.losses["nce"], patchnce.MultilayerPatchNCELoss) and cut.reduction == "mixed"
    epoch = epoch_iteration.initialize_epoch_iteration({"type": "SupervisedCycleGanEpoch", "data": "train", "criterion": "default", "pool_size": 50},
                                                       default_criterion=crit)
    assert epoch.criterion is crit and epoch.fake_X_pool.pool_size == 50
    x = torch.zeros(2, 3, 4, 4)
    assert epoch.fake_X_pool.query(x) is x                                           # a fresh pool returns its input
    with pytest.raises(ValueError):
        epoch_iteration.initialize_epoch_iteration({"type": "SupervisedCUTEpoch", "criterion": "default"})
    hed = epoch_iteration.initialize_epoch_iteration({"type": "SupervisedHEDGANEpoch", "criterion": FX.criterion_params("SupervisedHEDGANEpoch")})
    assert list(hed.criterion.losses) == ["adversarial", "edge"]
    with pytest.raises(NotImplementedError):
        epoch_iteration.gan_epochs.SupervisedGanEpoch(crit).step_losses({}, x, x)


def test_handled_manually_criteria_refuse_forward():
    from gandtr_amd.components.optim.criterion import compound
    cycle = compound.initialize_gan_criterion(FX.criterion_params("SupervisedCycleGanEpoch"))
    with pytest.raises(NotImplementedError, match="Losses are handled manually through SupervisedCycleGanEpoch"):
        cycle.forward(torch.zeros(1))
    bag = compound.initialize_gan_criterion({"loss": "loss_set", "first": {"loss": "l1"}, "second": {"loss": "mse", "reduction": "sum"}})
    assert bag.loss_names == {"first", "second"} and isinstance(bag.first, compound.L1Loss) and bag.second.reduction == "sum" and bag.reduction == "mixed"
    with pytest.raises(NotImplementedError, match="Losses are handled manually through epoch iteration"):
        bag.forward(torch.zeros(1))


def test_weight_keys_must_match_the_losses():
    from gandtr_amd.components.optim.criterion import compound
    with pytest.raises(AssertionError):
        compound.MultiheadLoss({"a": 1, "c": 1}, False, a={"loss": "l1"}, b={"loss": "l1"})
    with pytest.raises(AssertionError):
        compound.CombinationLoss({"a": 1}, True, a={"loss": "l1"}, b={"loss": "mse"})
    both = compound.MultiheadLoss(2, True, a={"loss": "l1"}, b={"loss": "mse", "reduction": "sum"})
    assert both.weights == {"a": 0.5, "b": 0.5} and both.reduction == "mixed"


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    """every refusal happens before any HIP call"""
    from gandtr_amd import _hip
    lib = _hip.load()
    maps = (ctypes.c_float * 64)()
    out = (ctypes.c_double * 8)()
    addr = ctypes.addressof(maps)

    def table(n=1, **kw):
        f = dict(a=addr, b=addr, target=0.0, kind=0, flags=0, n_images=2, count=64, weight=1.0)
        f.update(kw)
        return (_hip.MapLossPair * max(n, 1))(*[_hip.MapLossPair(**f) for _ in range(max(n, 1))])

    def run(n=1, per_image=out, per_pair=out, total=out, ws=out, ws_bytes=64, **kw):
        return lib.gdt_map_loss(table(n, **kw), n, per_image, per_pair, total, ws, ws_bytes, None)

    nbytes = ctypes.c_size_t()
    assert lib.gdt_map_loss_workspace_bytes(table(), 1, ctypes.byref(nbytes)) == _hip.GDT_OK and nbytes.value == (2 + 2) * 8
    big = table(count=3 * 8193, n_images=3)
    assert lib.gdt_map_loss_workspace_bytes(big, 1, ctypes.byref(nbytes)) == _hip.GDT_OK and nbytes.value == (3 * 2 + 3) * 8
    bad = [run(n=0), run(n=_hip.MAP_LOSS_MAX_PAIRS + 1), run(count=0), run(count=-4), run(count=63, n_images=2), run(n_images=0), run(kind=2), run(kind=-1),
           run(flags=2), run(flags=-1), run(a=None), run(a=addr + 2), run(per_image=None), run(per_pair=None), run(total=None), run(ws=None),
           run(ws_bytes=(2 + 2) * 8 - 1), lib.gdt_map_loss(None, 1, out, out, out, out, 64, None),
           lib.gdt_map_loss_workspace_bytes(table(), 1, None), lib.gdt_map_loss_workspace_bytes(table(), 0, ctypes.byref(nbytes)),
           lib.gdt_map_loss_workspace_bytes(table(count=7, n_images=2), 1, ctypes.byref(nbytes))]
    assert bad == [_hip.GDT_ERR_INVALID] * len(bad)
    with pytest.raises(ValueError, match="workspace too small"):
        _hip.check(run(ws_bytes=8))
    with pytest.raises(ValueError, match="n_images"):
        _hip.check(run(count=63))


@pytest.mark.parametrize("i", range(len(FX.CRITERION_SHAPES)))
def test_l1_and_mse_on_the_cpu_against_the_float64_cases(i):
    """non-negative terms: a reordered float64 sum moves the result by at most count * 2^-53 relative"""
    from gandtr_amd.components.optim.criterion import compound
    g = FX.gold()
    a, b = (t.double() for t in FX.criterion_maps(i))
    tol = a.numel() * EPS53
    for label, key, kwargs in (("l1", "c%d_l1", {}), ("mse", "c%d_mse", {}), ("l1", "c%d_l1_sum", {"reduction": "sum"})):
        crit = compound.initialize_gan_criterion({"loss": label, **kwargs})
        want = float(g[key % i])
        got = crit(a, b)
        assert got.dim() == 0 and got.dtype == torch.float64 and abs(float(got) - want) <= tol * abs(want)
        many = crit.evaluate_many([(a, b), (b, a)])
        assert many.shape == (2,) and many.dtype == torch.float64 and all(abs(float(v) - want) <= tol * abs(want) for v in many)
    af, bf = FX.criterion_maps(i)
    assert torch.equal(compound.L1Loss()(af, bf), torch.nn.functional.l1_loss(af, bf))               # fp32 CPU tensors: torch's op
    assert torch.equal(compound.MSELoss(reduction="none")(af, bf), (af - bf) ** 2)
    const = compound.map_losses([compound.MapPair(a, 1.0, "mse", False, 2.0), compound.MapPair(a, b, "l1", True, 1.0)])
    assert abs(float(const.per_pair[0]) - float(((a - 1.0) ** 2).mean())) <= tol * float(const.per_pair[0])
    assert abs(float(const.per_pair[1]) - float((torch.sigmoid(a) - torch.sigmoid(b)).abs().mean())) <= tol * float(const.per_pair[1]) + 2.0 ** -52
    assert float(const.total) == 2.0 * float(const.per_pair[0]) + float(const.per_pair[1])
    assert [tuple(t.shape) for t in const.per_image] == [(a.shape[0],)] * 2


def test_multihead_and_combination_on_the_cpu_against_the_float64_cases():
    from gandtr_amd.components.optim.criterion import compound
    g = FX.gold()
    for i, (weights, normalize, heads) in enumerate(FX.MULTIHEAD_CASES):
        crit = compound.initialize_gan_criterion(FX.multihead_params("multihead_loss", weights, normalize, heads))
        maps = {key: [t.double() for t in FX.criterion_maps(v[1])] for key, v in heads.items()}
        out = crit({key: m[0] for key, m in maps.items()}, {key: m[1] for key, m in maps.items()})
        assert list(out.partial) == [str(k) for k in g["m%d_keys" % i]] and crit.reduction == str(g["m%d_reduction" % i])
        count = max(m[0].numel() for m in maps.values())
        for got, want in zip(list(out.partial.values()) + [out.total], list(g["m%d_partial" % i]) + [g["m%d_total" % i]]):
            assert abs(float(got) - float(want)) <= (count + len(heads)) * EPS53 * abs(float(want))
    for i, (weights, normalize, heads, at) in enumerate(FX.COMBINATION_CASES):
        crit = compound.initialize_gan_criterion(FX.multihead_params("combination_loss", weights, normalize, heads))
        a, b = (t.double() for t in FX.criterion_maps(at))
        out = crit(a, b)
        assert list(out.partial) == [str(k) for k in g["k%d_keys" % i]]
        for got, want in zip(list(out.partial.values()) + [out.total], list(g["k%d_partial" % i]) + [g["k%d_total" % i]]):
            assert abs(float(got) - float(want)) <= (a.numel() + len(heads)) * EPS53 * abs(float(want))


@pytest.mark.parametrize("i", range(len(FX.STEP_CASES)))
def test_step_losses_on_float64_cpu_modules_against_the_reference(i):
    g = FX.gold()
    name, label = FX.STEP_CASES[i][:2]
    p = name + "_"
    nets = mirror_networks(i)
    for net in nets.values():
        (net.model if hasattr(net, "network_params") else net).double()
    X, Y = (t.double() for t in FX.step_inputs(i))
    epoch = mirror_epoch(label)
    losses, dbg = epoch.step_losses(nets, X, Y, patch_ids=cut_ids(p) if label == "SupervisedCUTEpoch" else None)
    assert list(losses) == [str(k) for k in g[p + "keys"]]                           # the reference's keys in the reference's order
    values = losses.item()
    assert list(values) == list(losses) and all(isinstance(v, float) for v in values.values())
    for key, want in zip(losses, g[p + "f64"]):
        assert losses[key].dim() == 0 and losses[key].dtype == torch.float64
        rel = abs(values[key] - float(want)) / abs(float(want))
        assert rel <= 1e-9, (key, values[key], float(want), rel)
    expected = {"SupervisedHEDNGANEpoch": ["real_X", "real_Y", "fake_Y", "real_E", "fake_E", "real_E_check"],
                "SupervisedHEDGANEpoch": ["real_X", "real_Y", "fake_Y", "real_E", "fake_E"],
                "SupervisedCycleGanEpoch": ["real_X", "fake_Y", "rec_X", "real_Y", "fake_X", "rec_Y"],
                "SupervisedCUTEpoch": ["real_X", "real_Y", "fake_Y", "idt_Y"]}[label]
    assert list(dbg) == expected and all(t.dim() == 3 for t in dbg.values())
    assert torch.equal(dbg["real_X"], X[-1]) and torch.equal(dbg["real_Y"], Y[-1])
    if "real_E" in dbg:
        assert 0.0 <= float(dbg["real_E"].min()) and float(dbg["fake_E"].max()) <= 1.0


def test_cut_refuses_the_weights_the_reference_cannot_log():
    from gandtr_amd.components.optim.criterion import compound
    from gandtr_amd.learning.epoch_iteration import cut_epochs
    params = FX.criterion_params("SupervisedCUTEpoch")
    params["weights"]["identity"] = 0
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(NotImplementedError):
        cut_epochs.SupervisedCutEpoch(compound.initialize_gan_criterion(params)).step_losses({"generator_X": None, "discriminator_Y": None, "featdown": None}, x, x)
