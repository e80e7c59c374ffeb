"""Shared by tests/golden/make_gan_objective_golden.py, test_gan_objective_host.py and test_hip_gan_objective.py: the cases of tests/golden/gan_objective.npz
(built from seeds with whichever module namespace the caller hands in: the reference's for the fixture, this repository's for the tests), the scenarios'
criterion sections, and the gates of the step cases (no test in here).

Gates.  ``emu_<map>`` of the fixture is max |map(reference) - map(the same reference with every conv weight and conv input rounded to fp16)| over the whole
chain of networks that produces the map; e(m) = 3 * emu_m -- the factor tests/test_hip_patchnce.py settled on for an f16 chain through the generator.
  l1 term of maps a, b with weight w:            w (e(a) + e(b))                       (|a' - b'| - |a - b| <= |a' - a| + |b' - b|, on every value)
  the same behind the sigmoid flag:              the same with the emu of the post-sigmoid maps
  mse against a constant, loss L, weight w:      w e(x) (2 sqrt(L / w) + e(x))         (mean (x + d - t)^2 - mean (x - t)^2 = mean 2 d (x - t) + mean d^2,
                                                                                        mean |x - t| <= sqrt(mean (x - t)^2) = sqrt(L / w))
  sums of terms (``total``, ``*_total``):        the sum of the parts' gates with the parts' coefficients
  CUT's patch-NCE terms:                         3 * f16_emulated_row_err of the layer (a mean of rows moves by at most the largest row error), carried
                                                 through the weights and the 0.5 of cut_epochs.py:66-68
Every gate is made of the reference's values and IEEE rounding alone."""
import math
import os
from collections import OrderedDict

import numpy as np
import torch

from gandtr_amd.tools import synth

GOLD_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gan_objective.npz")
_GOLD = []


def gold():
    if not _GOLD:
        _GOLD.append(np.load(GOLD_PATH))
    return _GOLD[0]


FACTOR = 3.0
NCE_LAYERS, NUM_PATCHES = "4,8,12,16", 64
D_GAIN = 0.2                       # N(0, 0.2) discriminator weights with InstanceNorm keep the activations O(1) (make_discriminator_golden.py)
RCFNGAN_WRAPPERS = ("meanstd_pre:[[0.5,0.5,0.5],[0.5,0.5,0.5]]:[[0.0,0.0,0.0],[1.0,1.0,1.0]],rgb2bgr_pre,"
                    "meanstd_pre:[[0.0,0.0,0.0],[255.0,255.0,255.0]]:[[104.00698793,116.66876762,122.67891434],[1.0,1.0,1.0]]")

# ---- criterion cases: (name, shape); maps a, b: N(0, 1) * 2 from seeds 200 + i
CRITERION_SHAPES = ((3, 1, 7, 11), (2, 3, 13, 9), (1, 1, 5, 5), (5, 2, 33, 31), (1, 3, 1, 1))
MULTIHEAD_CASES = (                # (weights, normalize_weights, {head: (loss label, index into CRITERION_SHAPES)})
    ({"adversarial": 1, "cycle": 10}, False, OrderedDict([("adversarial", ("mse", 0)), ("cycle", ("l1", 1))])),
    (0.5, False, OrderedDict([("a", ("l1", 2)), ("b", ("l1", 3)), ("c", ("mse", 4))])),
    ({"edge": 5, "hed": 1, "x": 2}, True, OrderedDict([("edge", ("l1", 3)), ("hed", ("l1", 0)), ("x", ("mse", 1))])),
)
COMBINATION_CASES = (              # (weights, normalize_weights, {name: loss label}, index into CRITERION_SHAPES)
    ({"first": 1, "second": 3}, False, OrderedDict([("first", "l1"), ("second", "mse")]), 3),
    (2, True, OrderedDict([("p", "mse"), ("q", "l1"), ("r", "l1")]), 1),
)


def criterion_maps(i):
    shape = CRITERION_SHAPES[i]
    return synth._normal(200 + i, "crit.a", shape, 2.0), synth._normal(200 + i, "crit.b", shape, 2.0)


def multihead_params(label, weights, normalize, heads):
    return {"loss": label, "weights": dict(weights) if isinstance(weights, dict) else weights, "normalize_weights": normalize,
            **{key: {"loss": v[0] if isinstance(v, tuple) else v} for key, v in heads.items()}}


# ---- step cases: (name, EPOCH_ITERATIONS label, norm of generator and discriminator, input shape, detector)
STEP_CASES = (
    ("hedngan_batch", "SupervisedHEDNGANEpoch", "batch", (2, 3, 40, 52), "hed"),
    ("hedngan_instance", "SupervisedHEDNGANEpoch", "instance", (1, 3, 24, 28), "hed"),
    ("hedgan_batch", "SupervisedHEDGANEpoch", "batch", (2, 3, 40, 52), "hed"),
    ("cyclegan_0", "SupervisedCycleGanEpoch", "instance", (2, 3, 40, 52), None),
    ("cyclegan_1", "SupervisedCycleGanEpoch", "instance", (1, 3, 24, 28), None),
    ("cut_0", "SupervisedCUTEpoch", "instance", (2, 3, 40, 52), None),
    ("rcfngan_batch", "SupervisedHEDNGANEpoch", "batch", (2, 3, 64, 96), "rcf"),
    ("cyclegan_plain", "SupervisedCycleGanEpoch", "instance", (2, 3, 40, 52), None),
)
CUT_IDS_SEED = 95
# the student detector's weights: of the seeds 1 .. 6 the one whose E_real and E_fake lie furthest apart against their gates (seed 1: 1.6e-2 apart against
# 4.1e-2 of gates at (2, 3, 40, 52) -- a test that could not tell the two terms apart; seed 5: 8.9e-1 against 5.7e-2); the teacher has seed 0
STUDENT_SEED = 5
# CycleGAN's second generator has N(0, 0.001) conv weights: behind InstanceNorm only the last conv's gain shows, so its pictures are near zero, rec_X with
# them, and the two cycle terms lie apart (6.32 and 7.26 against 0.84 of gates; with 0.02 for both generators: 7.53 and 7.29 against 1.66)
CYCLE_Y_GAIN = 0.001
# ... which leaves that generator's own pictures near zero.  One more CycleGAN case gives both generators the ordinary 0.02: it checks every loss against its
# gate with a second generator whose pictures are O(1), and is exempt from the lie-apart condition (its two cycle terms are 7.53 and 7.29)
PLAIN_GAIN_CASES = ("cyclegan_plain",)

_ADV = {"loss": "discriminator_loss", "criterion": {"loss": "mse"}}
_CYCLE_G = {"loss": "multihead_loss", "weights": {"adversarial": 1, "cycle": 10}, "normalize_weights": False, "adversarial": {"loss": "mse"},
            "cycle": {"loss": "l1"}}


def criterion_params(label):
    """the criterion sections of train_hedgan.yml / train_hedngan.yml / train_cyclegan.yml / train_cut.yml (num_patches 64 for the small maps); a fresh
    nested dict on every call: the reference pops from it"""
    import copy
    if label == "SupervisedHEDNGANEpoch":
        p = {"loss": "multihead_loss", "weights": {"adversarial": 1, "edge": 5, "hed": 1}, "normalize_weights": False, "adversarial": _ADV,
             "edge": {"loss": "l1"}, "hed": {"loss": "l1"}}
    elif label == "SupervisedHEDGANEpoch":
        p = {"loss": "multihead_loss", "weights": {"adversarial": 1, "edge": 5}, "normalize_weights": False, "adversarial": _ADV, "edge": {"loss": "l1"}}
    elif label == "SupervisedCycleGanEpoch":
        p = {"loss": "cycle_loss", "loss_G_X": copy.deepcopy(_CYCLE_G), "loss_G_Y": copy.deepcopy(_CYCLE_G), "loss_D_X": copy.deepcopy(_ADV),
             "loss_D_Y": copy.deepcopy(_ADV)}
    elif label == "SupervisedCUTEpoch":
        p = {"loss": "multihead_loss", "weights": {"adversarial": 1, "identity": 10, "nce": 1}, "normalize_weights": False, "adversarial": _ADV,
             "identity": {"loss": "l1"}, "nce": {"loss": "multilayer_patchnce_loss", "batch_dim_for_bmm": 1, "nce_layers": NCE_LAYERS,
                                                 "num_patches": NUM_PATCHES, "temperature": 0.07, "weight": 1}}
    else:
        raise KeyError(label)
    return copy.deepcopy(p)


def step_inputs(i):
    shape = STEP_CASES[i][3]
    return synth.synth_input(300 + i, shape, 1.0, name="src"), synth.synth_input(300 + i, shape, 1.0, name="tgt")


def step_networks(i, p2p, hed_cls, make_rcf):
    """the case's networks in eval mode with their seeded weights: ``p2p`` a module with ResnetGenerator / NLayerDiscriminator / PatchSampleF, ``hed_cls``
    the HED class, ``make_rcf(state)`` -> an RCF detector behind the rcfngan wrapper chain (a SingleNetwork)"""
    name, label, norm, shape, detector = STEP_CASES[i]

    def gen(seed, gain=0.02):
        net = p2p.ResnetGenerator(3, 3, norm_layer=norm).eval()
        net.load_state_dict(synth.generator_state(seed, norm, gain=gain))
        return net

    def disc(seed):
        net = p2p.NLayerDiscriminator(3, norm_layer=norm).eval()
        net.load_state_dict(synth.discriminator_state(seed, norm, gain=D_GAIN))
        return net

    def det(seed):
        if detector == "rcf":
            return make_rcf(synth.rcf_state(seed))
        net = hed_cls().eval()
        net.load_state_dict(synth.hed_state(seed))
        return net

    nets = OrderedDict(generator_X=gen(0))
    if label == "SupervisedCycleGanEpoch":
        nets.update(generator_Y=gen(1, 0.02 if name in PLAIN_GAIN_CASES else CYCLE_Y_GAIN), discriminator_X=disc(40), discriminator_Y=disc(41))
        return nets
    nets["discriminator_Y"] = disc(41)
    if label == "SupervisedCUTEpoch":
        netF = p2p.PatchSampleF(use_mlp=True, input_nc=None, nc=256, nce_layers=None)
        netF.create_mlp([torch.zeros(1, c, 1, 1) for c in (128, 256, 256, 256)], "cpu")
        netF.load_state_dict(synth.patchsample_state(90, (128, 256, 256, 256), 256))
        nets["featdown"] = netF.eval()
        return nets
    nets["detector"] = det(STUDENT_SEED)
    if label == "SupervisedHEDNGANEpoch":
        nets["detector_frozen"] = det(0)
    return nets


# ---- gates
def _mse_gate(w, ex, loss):
    return w * ex * (2.0 * math.sqrt(max(loss, 0.0) / w) + ex)


def step_gates(i, g=None):
    """{key: gate} of step case i from the fixture's fp32 losses and emu figures"""
    g = g or gold()
    name, label = STEP_CASES[i][:2]
    p = name + "_"
    L = dict(zip([str(k) for k in g[p + "keys"]], [float(v) for v in g[p + "f32"]]))
    e = lambda m: FACTOR * float(g[p + "emu_" + m])
    w = criterion_params(label)
    gates = {}
    if label != "SupervisedCycleGanEpoch":
        wa = w["weights"]["adversarial"]
        gates["D_real"] = _mse_gate(wa, e("pred_real"), L["D_real"])
        gates["D_fake"] = _mse_gate(wa, e("pred_fake"), L["D_fake"])
        gates["G_gan"] = _mse_gate(wa, e("pred_fake"), L["G_gan"])
    if label == "SupervisedHEDNGANEpoch":
        gates["E_real"] = w["weights"]["hed"] * (e("real_M") + e("target_M"))
        gates["E_fake"] = w["weights"]["hed"] * (e("fake_M") + e("target_M"))
        gates["G_hed"] = w["weights"]["edge"] * (e("sig_fake_M") + e("sig_target_M"))
        gates["total"] = gates["G_gan"] + gates["G_hed"] + 0.5 * (gates["D_real"] + gates["D_fake"])
    elif label == "SupervisedHEDGANEpoch":
        gates["G_hed"] = w["weights"]["edge"] * (e("sig_fake_M") + e("sig_real_M"))
        gates["total"] = gates["G_gan"] + gates["G_hed"] + 0.5 * (gates["D_real"] + gates["D_fake"])
    elif label == "SupervisedCycleGanEpoch":
        gates["total"] = 0.0
        for s in ("X", "Y"):
            ws = w["loss_G_" + s]["weights"]
            gates["netG_%s_adversarial" % s] = _mse_gate(ws["adversarial"], e("pred_%s_fake" % s), L["netG_%s_adversarial" % s])
            gates["netG_%s_cycle" % s] = ws["cycle"] * e("rec_" + s)
            gates["netG_%s_total" % s] = gates["netG_%s_adversarial" % s] + gates["netG_%s_cycle" % s]
            gates["netD_%s_total" % s] = 0.5 * (_mse_gate(1.0, e("pred_%s_real" % s), float(g[p + "aux_D_%s_real" % s])) +
                                                _mse_gate(1.0, e("pred_%s_fake" % s), float(g[p + "aux_D_%s_fake" % s])))
            gates["total"] += gates["netG_%s_total" % s] + gates["netD_%s_total" % s]
    else:
        w_idt, w_nce = w["weights"]["identity"], w["nce"]["weight"]
        err_nce, err_idt = FACTOR * g[p + "nce_f16_emulated_row_err"], FACTOR * g[p + "idt_f16_emulated_row_err"]
        layers = [int(v) for v in NCE_LAYERS.split(",")]
        for l, layer in enumerate(layers):
            gates["G_idt_layer%d" % layer] = w_idt * float(err_idt[l])
            gates["G_nce_layer%d" % layer] = 0.5 * (w_nce * float(err_nce[l]) + w_idt * float(err_idt[l]))
        gates["G_idt"] = w_idt * float(err_idt.mean())
        gates["G_nce"] = 0.5 * (w_nce * float(err_nce.mean()) + w_idt * float(err_idt.mean()))
        gates["total"] = gates["G_gan"] + gates["G_nce"] + 0.5 * (gates["D_real"] + gates["D_fake"])
    assert set(gates) == set(L), set(gates) ^ set(L)
    return gates, L


# losses a wiring mistake would exchange: they must differ by more than the sum of their gates, or the device gate proves nothing about the wiring
EXCHANGEABLE = {
    "SupervisedHEDNGANEpoch": (("D_real", "D_fake"), ("E_real", "E_fake")),
    "SupervisedHEDGANEpoch": (("D_real", "D_fake"),),
    "SupervisedCUTEpoch": (("D_real", "D_fake"),),
    "SupervisedCycleGanEpoch": (("netG_X_adversarial", "netG_Y_adversarial"), ("netG_X_cycle", "netG_Y_cycle"), ("netG_X_total", "netG_Y_total"),
                                ("netD_X_total", "netD_Y_total")),
}


# ---- this repository's side of the cases
EPS53 = 2.0 ** -53


def mirror_rcf(state, device="cpu"):
    from gandtr_amd.learning import network as N
    params = {"type": "SingleNetwork", "model": {"architecture": "rcf"}, "initialize": False, "runtime": {"wrappers": RCFNGAN_WRAPPERS}}
    net = N.initialize_network(params, device).eval()
    net.model.load_state_dict(state)
    return net


def mirror_networks(i):
    from gandtr_amd.components.model.network import hed, p2p_networks
    return step_networks(i, p2p_networks, hed.HedInterpolation, mirror_rcf)


def mirror_epoch(label):
    from gandtr_amd.components.optim.criterion import compound
    from gandtr_amd.learning import epoch_iteration
    return epoch_iteration.EPOCH_ITERATIONS[label](compound.initialize_gan_criterion(criterion_params(label)))


def cut_ids(p):
    g = gold()
    return tuple([torch.from_numpy(g[p + "ids_%s%d" % (tag, l)].astype("int64")) for l in range(4)] for tag in ("nce", "idt"))
