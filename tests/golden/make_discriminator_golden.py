"""Generate tests/golden/discriminator.npz by IMPORTING THE REFERENCE's NLayerDiscriminator and DiscriminatorLoss (read-only) -- the way make_golden.py does.

Runs only where the reference is present.  Weights and inputs are regenerated from seeds on the consumer side (gandtr_amd.tools.synth:
``discriminator_state`` filled into the reference module with a strict ``load_state_dict``, so its key list is the reference's; InstanceNorm cases
with N(0, 0.2) conv weights -- the gain that keeps the activations O(1) --, BatchNorm cases with kaiming weights and non-trivial running statistics
and affine parameters).  Stored per case: the seeds and shapes, the reference's fp32 logit map, its ``DiscriminatorLoss`` values (mse; real and fake
target) and ``f16_emulated_err``: max|fp32 logits - emulated logits| / max|fp32 logits|, where the emulation is the SAME reference module evaluated on
the CPU with every conv weight and every conv input rounded to fp16 (fp32 accumulation) -- a figure made of the reference and IEEE rounding alone.
Also stored: the state_dict key list and shapes of every configuration and the reference's parameter count of the ndf = 64, n_layers = 3 net.

usage:  python tests/golden/make_discriminator_golden.py
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden                                             # noqa: E402  (placeholders, paths)
from gandtr_amd.tools import synth                             # noqa: E402

GAIN = 0.2
# (ndf, n_layers, norm, input shape); weights seed 40 + i, input seed 50 + i
CASES = ((64, 3, "instance", (2, 3, 40, 52)), (64, 3, "batch", (2, 3, 40, 52)), (64, 3, "instance", (3, 3, 70, 94)), (64, 3, "batch", (3, 3, 70, 94)),
         (16, 2, "instance", (2, 3, 40, 52)))


def case_state(i):
    ndf, n_layers, norm, _ = CASES[i]
    return synth.discriminator_state(40 + i, norm, ndf=ndf, n_layers=n_layers, gain=GAIN)


def case_input(i):
    return synth.synth_input(50 + i, CASES[i][3], 1.0)


def f16_emulation(model):
    """a copy of ``model`` whose convs see fp16-rounded weights and fp16-rounded inputs (fp32 arithmetic otherwise)"""
    m = copy.deepcopy(model)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Conv2d):
            mod.weight.data = mod.weight.data.half().float()
            mod.register_forward_pre_hook(lambda _m, args: (args[0].half().float(),))
    return m


def main():
    make_golden._install_placeholders()
    sys.path.insert(0, make_golden.REF)
    threads = torch.get_num_threads()
    import mdir                                                     # noqa: F401
    torch.set_num_threads(threads)
    from mdir.components.model.network import p2p_networks as ref_p2p
    from mdir.components.optim.criterion import compound_losses as ref_losses

    T = lambda t: t.detach().cpu().numpy()
    arrays = {"n_cases": np.int64(len(CASES)), "gain": np.float64(GAIN)}
    crit = ref_losses.DiscriminatorLoss({"loss": "mse"})
    with torch.no_grad():
        for i, (ndf, n_layers, norm, shape) in enumerate(CASES):
            model = ref_p2p.NLayerDiscriminator(3, ndf=ndf, n_layers=n_layers, norm_layer=norm).eval()
            model.load_state_dict(case_state(i))
            p = "c%d_" % i
            arrays[p + "cfg"] = np.array([ndf, n_layers, 40 + i, 50 + i], dtype=np.int64)
            arrays[p + "norm"] = np.array(norm)
            arrays[p + "shape"] = np.array(shape, dtype=np.int64)
            arrays[p + "keys"] = np.array(list(model.state_dict().keys()))
            arrays[p + "shapes"] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in model.state_dict().values()], dtype=np.int64)
            x = case_input(i)
            y = model(x)
            arrays[p + "logits"] = T(y)
            arrays[p + "loss_real"] = T(crit(y, True, "cpu").total)
            arrays[p + "loss_fake"] = T(crit(y, False, "cpu").total)
            emu = f16_emulation(model)(x)
            err = float((emu - y).abs().max() / y.abs().max())
            arrays[p + "f16_emulated_err"] = np.float64(err)
            print("case %d ndf %d n_layers %d %s %s: logits %s max|y| %.3f  loss real %.4f fake %.4f  f16_emulated_err %.3e" %
                  (i, ndf, n_layers, norm, shape, tuple(y.shape), float(y.abs().max()), arrays[p + "loss_real"], arrays[p + "loss_fake"], err))
        full = ref_p2p.NLayerDiscriminator(3, ndf=64, n_layers=3, norm_layer="instance")
        arrays["param_count_ndf64_l3_instance"] = np.int64(sum(p.numel() for p in full.parameters()))
        print("parameters (ndf 64, n_layers 3, instance): %d" % arrays["param_count_ndf64_l3_instance"])
    path = os.path.join(HERE, "discriminator.npz")
    np.savez_compressed(path, **arrays)
    print("wrote discriminator.npz %.1f KiB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
