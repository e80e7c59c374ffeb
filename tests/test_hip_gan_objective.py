"""The GAN scenarios' objectives on the device: the compound criteria against the float64 criterion cases, and ``step_losses`` of the four scenarios against the
reference's fp32 step values of tests/golden/gan_objective.npz -- keys and order, the derived gates, bit-identical repeats, the number of graph runs.

Gates: tests/gan_objective_fixture.py (3 x the fixture's fp16 emulation error of every map a term reads, carried through the term; nothing from the device).
Default precisions: generator f16c; discriminator, HED and RCF f16.  The same cases also run with every network in f16x3 against the same gates.

Measured on an MI355X, largest measured / gate over the keys of a case (the test prints the ratio of every key) -- default precisions: hedngan_batch 0.029,
hedngan_instance 0.251 (D_fake, G_gan), hedgan_batch 0.016, cyclegan_0 0.008, cyclegan_1 0.604 (netD_Y_total; netG_X_adversarial 0.475), cut_0 0.021,
rcfngan_batch 0.015, cyclegan_plain 0.021; f16x3: at most 0.001 on every case."""
import pytest
import torch

import gan_objective_fixture as FX
from gan_objective_fixture import EPS53, cut_ids, mirror_epoch, mirror_rcf

pytestmark = pytest.mark.gpu

GRAPH_RUNS = {"SupervisedHEDNGANEpoch": 4, "SupervisedHEDGANEpoch": 3, "SupervisedCycleGanEpoch": 6, "SupervisedCUTEpoch": 4}


def _device_networks(i, dev, precision=None):
    from gandtr_amd.components.model.network import hed, p2p_networks
    nets = FX.step_networks(i, p2p_networks, hed.HedInterpolation, lambda state: mirror_rcf(state, dev))
    for key, net in nets.items():
        module = net.model if hasattr(net, "network_params") else net
        if precision is not None:
            module.hip_precision = precision
        if module is net:
            nets[key] = net.to(dev)
    return nets


def test_criteria_on_the_device_against_the_float64_cases(cuda_device, monkeypatch):
    from gandtr_amd.components.optim.criterion import compound
    g = FX.gold()
    for i in range(len(FX.CRITERION_SHAPES)):
        a, b = (t.to(cuda_device) for t in FX.criterion_maps(i))
        for label, key in (("l1", "c%d_l1"), ("mse", "c%d_mse")):
            want = float(g[key % i])
            crit = compound.initialize_gan_criterion({"loss": label})
            got64 = crit.evaluate_many([(a, b)])
            assert got64.is_cuda and got64.dtype == torch.float64 and abs(float(got64[0].cpu()) - want) <= a.numel() * EPS53 * want
            got = crit(a, b)
            assert got.is_cuda and got.dtype == torch.float32 and got.dim() == 0 and abs(float(got.cpu()) - want) <= 2.0 ** -24 * want
        want = float(g["c%d_l1_sum" % i])
        assert abs(float(compound.L1Loss(reduction="sum")(a, b).cpu()) - want) <= 2.0 ** -23 * want
    calls = []
    real = compound.map_losses
    monkeypatch.setattr(compound, "map_losses", lambda pairs: calls.append(len(pairs)) or real(pairs))
    for i, (weights, normalize, heads) in enumerate(FX.MULTIHEAD_CASES):
        crit = compound.initialize_gan_criterion(FX.multihead_params("multihead_loss", weights, normalize, heads))
        maps = {key: [t.to(cuda_device) for t in FX.criterion_maps(v[1])] for key, v in heads.items()}
        del calls[:]
        out = crit({key: m[0] for key, m in maps.items()}, {key: m[1] for key, m in maps.items()})
        assert calls == [len(heads)]                                                  # all heads in ONE call
        assert list(out.partial) == [str(k) for k in g["m%d_keys" % i]] and out.total.is_cuda and out.total.dtype == torch.float32
        for got, want in zip(out.partial.values(), g["m%d_partial" % i]):
            assert abs(float(got.cpu()) - float(want)) <= 2.0 ** -23 * float(want)
        assert abs(float(out.total.cpu()) - float(g["m%d_total" % i])) <= (len(heads) + 1) * 2.0 ** -24 * float(g["m%d_total" % i])
    for i, (weights, normalize, heads, at) in enumerate(FX.COMBINATION_CASES):
        crit = compound.initialize_gan_criterion(FX.multihead_params("combination_loss", weights, normalize, heads))
        a, b = (t.to(cuda_device) for t in FX.criterion_maps(at))
        del calls[:]
        out = crit(a, b)
        assert calls == [len(heads)] and list(out.partial) == [str(k) for k in g["k%d_keys" % i]]
        for got, want in zip(list(out.partial.values()), list(g["k%d_partial" % i])):
            assert abs(float(got.cpu()) - float(want)) <= 2.0 ** -23 * float(want)
        assert abs(float(out.total.cpu()) - float(g["k%d_total" % i])) <= (len(heads) + 1) * 2.0 ** -24 * float(g["k%d_total" % i])


@pytest.mark.parametrize("precision", [None, "f16x3"], ids=["default", "f16x3"])
@pytest.mark.parametrize("i", range(len(FX.STEP_CASES)), ids=[c[0] for c in FX.STEP_CASES])
def test_step_losses_against_the_reference(cuda_device, monkeypatch, i, precision):
    from gandtr_amd import engine
    name, label = FX.STEP_CASES[i][:2]
    p = name + "_"
    gates, want = FX.step_gates(i)
    nets = _device_networks(i, cuda_device, precision)
    X, Y = (t.to(cuda_device) for t in FX.step_inputs(i))
    epoch = mirror_epoch(label)
    ids = cut_ids(p) if label == "SupervisedCUTEpoch" else None
    runs = []
    forward = engine.HipNet.forward
    monkeypatch.setattr(engine.HipNet, "forward", lambda self, *a, **k: runs.append(1) or forward(self, *a, **k))
    losses, dbg = epoch.step_losses(nets, X, Y, patch_ids=ids)
    assert len(runs) == GRAPH_RUNS[label], (len(runs), GRAPH_RUNS[label])
    assert list(losses) == [str(k) for k in FX.gold()[p + "keys"]]
    assert all(v.is_cuda and v.dtype == torch.float64 and v.dim() == 0 for v in losses.values())
    values = losses.item()
    worst = 0.0
    for key in losses:
        ratio = abs(values[key] - want[key]) / gates[key]
        worst = max(worst, ratio)
        print("%s %s %-22s device %.6f reference %.6f  measured / gate = %.3f (gate %.3e)" % (name, precision or "default", key, values[key], want[key],
                                                                                                ratio, gates[key]))
    print("%s %s: largest measured / gate = %.3f" % (name, precision or "default", worst))
    for key in losses:
        assert abs(values[key] - want[key]) <= gates[key], (key, values[key], want[key], gates[key])
    again, dbg2 = epoch.step_losses(nets, X, Y, patch_ids=ids)                        # two calls: identical bits
    assert list(again) == list(losses) and all(torch.equal(again[k], losses[k]) for k in losses)
    assert list(dbg) == list(dbg2) and all(torch.equal(dbg[k], dbg2[k]) for k in dbg) and all(t.is_cuda and t.dim() == 3 for t in dbg.values())
    if "real_E_check" in dbg:
        assert 0.0 <= float(dbg["real_E_check"].min()) and float(dbg["real_E"].max()) <= 1.0 and dbg["fake_E"].shape == dbg["real_E"].shape
