"""Generate tests/golden/unet.npz by IMPORTING THE REFERENCE's UnetGenerator and ReflectPadMakeDivisible (read-only) -- the way make_golden.py does.

Runs only where the reference is present.  Weights and inputs are regenerated from seeds on the consumer side (gandtr_amd.tools.synth: ``unet_state``
filled into the reference module with a strict ``load_state_dict``, so its key list is the reference's).  Gains: InstanceNorm cases N(0, 0.2) conv weights,
BatchNorm cases kaiming-scaled weights with non-trivial running statistics and affine parameters; the outermost up conv N(0, sqrt(2 / (4 cin))) in both --
max|pre-tanh| of every case lies in [0.5, 20] (asserted here, stored as ``pre_max``).

Stored per case: seeds, config, the key list and shapes, the reference's fp32 map in front of the Tanh (``pre``, whole), the Tanh output at every fourth
row and column (``tanh_sub`` = out[:, :, ::4, ::4]: the Tanh is elementwise, and the two whole maps of every case together would pass the size limit of a
committed file) and ``f16_emulated_err``: max|d pre| / max|pre| of the SAME reference module evaluated on the CPU with every Conv2d / ConvTranspose2d
input and weight rounded to fp16 (fp32 arithmetic otherwise); for BatchNorm cases the BatchNorm behind a conv is folded into its weight in fp32 BEFORE the
rounding, as the device builder does.  A figure made of the reference and IEEE rounding alone.

Wrapper record: the reference's ReflectPadMakeDivisible(32) on a (1, 3, 50, 70) tensor and on a list of that tensor and a (1, 2, 20, 33) one -- the padding
tuples, the padded tensors (the list's first is the single one's), the crop of the padded tensors -- and the reference wrapper + case-0 net on the
(1, 3, 50, 70) tensor: the cropped Tanh output, the range of the map in front of the Tanh and the emulation figure of that run.

usage:  python tests/golden/make_unet_golden.py
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
# (norm, num_downs, ngf, input shape, use_dropout); weights seed 60 + i, input seed 70 + i
CASES = (("instance", 5, 16, (2, 3, 64, 96), False), ("batch", 5, 16, (2, 3, 32, 64), False), ("instance", 5, 64, (2, 3, 64, 64), False),
         ("batch", 6, 64, (1, 3, 64, 64), False), ("batch", 5, 64, (1, 3, 96, 160), False), ("batch", 6, 16, (1, 3, 64, 128), True))
WRAP_SEED, WRAP_SHAPES = 80, ((1, 3, 50, 70), (1, 2, 20, 33))


def case_state(i):
    norm, num_downs, ngf, _, _ = CASES[i]
    return synth.unet_state(60 + i, norm, ngf=ngf, num_downs=num_downs, gain=GAIN)


def case_input(i):
    return synth.synth_input(70 + i, CASES[i][3], 1.0)


def wrap_inputs():
    return [synth.synth_input(WRAP_SEED + k, s, 1.0) for k, s in enumerate(WRAP_SHAPES)]


def f16_emulation(model):
    """a copy of ``model`` whose convs see fp16-rounded inputs and fp16-rounded weights -- with the BatchNorm2d that follows a conv folded into it first
    (scale into the weight in fp32, shift into the bias; the BatchNorm becomes the identity)"""
    m = copy.deepcopy(model).eval()
    convs = (torch.nn.Conv2d, torch.nn.ConvTranspose2d)
    for seq in [s for s in m.modules() if isinstance(s, torch.nn.Sequential)]:
        for k in range(len(seq) - 1):
            conv, bn = seq[k], seq[k + 1]
            if isinstance(conv, convs) and isinstance(bn, torch.nn.BatchNorm2d):
                s = (bn.weight.data / torch.sqrt(bn.running_var + bn.eps)).float()
                bias = conv.bias.data if conv.bias is not None else torch.zeros_like(s)
                conv.bias = torch.nn.Parameter(bn.bias.data + (bias - bn.running_mean) * s)
                shape = (1, -1, 1, 1) if isinstance(conv, torch.nn.ConvTranspose2d) else (-1, 1, 1, 1)
                conv.weight.data = conv.weight.data * s.reshape(shape)
                seq[k + 1] = torch.nn.Identity()
    for mod in m.modules():
        if isinstance(mod, convs):
            mod.weight.data = mod.weight.data.half().float()
            mod.register_forward_pre_hook(lambda _m, args: (args[0].half().float(),))
    return m


def pre_and_out(model, x):
    """(map in front of the Tanh, output) of one forward"""
    seen = []
    h = model.model.model[-2].register_forward_hook(lambda _m, _i, o: seen.append(o.clone()))
    y = model(x.clone())
    h.remove()
    return seen[0], y


def main():
    make_golden._install_placeholders()
    sys.path.insert(0, make_golden.REF)
    threads = torch.get_num_threads()
    import mdir                                                     # noqa: F401
    torch.set_num_threads(threads)
    from mdir.components.model.network import p2p_networks as ref_p2p
    from mdir.components.data import wrapper as ref_wrapper

    T = lambda t: t.detach().cpu().numpy()
    arrays = {"n_cases": np.int64(len(CASES)), "gain": np.float64(GAIN)}
    models = []
    with torch.no_grad():
        for i, (norm, num_downs, ngf, shape, dropout) in enumerate(CASES):
            model = ref_p2p.UnetGenerator(3, 3, num_downs, ngf=ngf, norm_layer=norm, use_dropout=dropout).eval()
            model.load_state_dict(case_state(i))
            models.append(model)
            p = "c%d_" % i
            arrays[p + "cfg"] = np.array([num_downs, ngf, int(dropout), 60 + i, 70 + i], dtype=np.int64)
            arrays[p + "norm"] = np.array(norm)
            arrays[p + "shape"] = np.array(shape, dtype=np.int64)
            arrays[p + "keys"] = np.array(list(model.state_dict().keys()))
            arrays[p + "shapes"] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in model.state_dict().values()], dtype=np.int64)
            x = case_input(i)
            pre, y = pre_and_out(model, x)
            pre_max = float(pre.abs().max())
            assert 0.5 <= pre_max <= 20.0, pre_max
            arrays[p + "pre"] = T(pre)
            arrays[p + "tanh_sub"] = T(y[:, :, ::4, ::4])
            arrays[p + "pre_max"] = np.float64(pre_max)
            emu, _ = pre_and_out(f16_emulation(model), x)
            err = float((emu - pre).abs().max() / pre.abs().max())
            arrays[p + "f16_emulated_err"] = np.float64(err)
            print("case %d %s num_downs %d ngf %d %s dropout %d: max|pre-tanh| %.3f  f16_emulated_err %.3e" % (i, norm, num_downs, ngf, shape, dropout, pre_max, err))
        # ---- the wrapper
        wrap = ref_wrapper.ReflectPadMakeDivisible(32, "cpu")
        xs = wrap_inputs()
        padded, padding = wrap.preprocess(xs[0], None)
        arrays["wrap_padding"] = np.array(padding, dtype=np.int64)
        arrays["wrap_padded"] = T(padded)
        assert torch.equal(wrap.postprocess(padded, None, padding), xs[0])                      # (the crop of the padded tensor is the input)
        lp, lpad = wrap.preprocess(list(xs), None)
        assert torch.equal(lp[0], padded) and tuple(lpad[0]) == tuple(padding)
        arrays["wrap_list_padding"] = np.array(lpad, dtype=np.int64)
        arrays["wrap_list_padded1"] = T(lp[1])
        crops = wrap.postprocess(lp, None, lpad)
        assert all(torch.equal(c, x) for c, x in zip(crops, xs))
        arrays["wrap_list_crop1"] = T(crops[1])
        pre, y = pre_and_out(models[0], padded)
        emu, _ = pre_and_out(f16_emulation(models[0]), padded)
        arrays["wrap_net_out"] = T(wrap.postprocess(y, None, padding))
        arrays["wrap_net_pre_max"] = np.float64(float(pre.abs().max()))
        arrays["wrap_net_f16_emulated_err"] = np.float64(float((emu - pre).abs().max() / pre.abs().max()))
        print("wrapper: padding %s list %s; wrapped net max|pre-tanh| %.3f f16_emulated_err %.3e" % (padding, lpad, arrays["wrap_net_pre_max"], arrays["wrap_net_f16_emulated_err"]))
    path = os.path.join(HERE, "unet.npz")
    np.savez_compressed(path, **arrays)
    print("wrote unet.npz %.1f KiB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
