"""Generate tests/golden/p2p_unet.npz by IMPORTING THE REFERENCE's unet.py (P2pUNet, OutconvP2pUNet, InconvP2pUNet, AlignedP2pUNet, ShallowP2pUNet) and
ReflectPadMakeDivisible (read-only) -- the way make_unet_golden.py does.

Runs only where the reference is present.  Weights and inputs are regenerated from seeds on the consumer side (gandtr_amd.tools.synth: ``p2p_unet_state``
filled into the reference module with a strict ``load_state_dict``, so its key list is the reference's).  max|map| of every case lies in [0.5, 20] (asserted
here, stored as ``map_max``); the map is the one in front of the Tanh where the net has one, else the output.

Stored per case: the label, the constructor arguments (names and values), the seeds, the input shape, the key list and shapes, the reference's fp32 output
(``out``), the map in front of the Tanh where there is one (``pre``) and ``f16_emulated_err``: max|d map| / max|map| of the SAME reference module evaluated on
the CPU with every Conv2d / ConvTranspose2d input and weight rounded to fp16 (fp32 arithmetic otherwise), the BatchNorm behind a conv folded into its weight
in fp32 BEFORE the rounding (make_unet_golden.f16_emulation).  A figure made of the reference and IEEE rounding alone.

Wrapper record: the reference's ReflectPadMakeDivisible(4) + the aligned net of case 6 on a (1, 3, 50, 70) tensor: the cropped output, the range of the map
and the emulation figure of that run.

usage:  python tests/golden/make_p2p_unet_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden                                             # noqa: E402  (placeholders, paths)
import make_unet_golden                                        # noqa: E402  (f16_emulation)
from gandtr_amd.tools import synth                             # noqa: E402

# (label, reference class, constructor arguments, input shape); weights seed 160 + i, input seed 170 + i
CASES = (("p2p_unet", "P2pUNet", dict(nested_levels=2), (2, 3, 24, 40)),
         ("p2p_unet", "P2pUNet", dict(nested_levels=5, batchnorm=True, dropout=0.5), (1, 3, 64, 128)),
         ("outconv_unet", "OutconvP2pUNet", dict(nested_levels=2), (2, 3, 24, 40)),
         ("outconv_unet", "OutconvP2pUNet", dict(nested_levels=0), (2, 4, 10, 14)),
         ("outconv_unet", "OutconvP2pUNet", dict(nested_levels=3, batchnorm=True, outconv_kernel=5), (1, 3, 32, 48)),
         ("inconv_p2p_unet", "InconvP2pUNet", dict(nested_levels=2), (2, 1, 24, 40)),
         ("aligned_p2p_unet", "AlignedP2pUNet", dict(nested_levels=2), (2, 3, 20, 36)),
         ("aligned_p2p_unet", "AlignedP2pUNet", dict(nested_levels=1), (2, 3, 10, 14)),
         ("shallow_p2p_unet", "ShallowP2pUNet", dict(nested_levels=2), (2, 3, 24, 40)),
         ("shallow_p2p_unet", "ShallowP2pUNet", dict(nested_levels=4), (1, 3, 64, 32)))
OUT_CHANNELS = 3
WRAP_CASE, WRAP_DIV, WRAP_SEED, WRAP_SHAPE = 6, 4, 190, (1, 3, 50, 70)


def case_state(i):
    label, _, cfg, shape = CASES[i]
    return synth.p2p_unet_state(label, 160 + i, in_channels=shape[1], out_channels=OUT_CHANNELS, **cfg)


def case_input(i):
    return synth.synth_input(170 + i, CASES[i][3], 1.0)


def map_and_out(model, x):
    """(map in front of the Tanh -- the output itself where the net has none --, output, whether there is a Tanh) of one forward"""
    tanh = isinstance(model.outerblock[-1], torch.nn.Tanh)
    if not tanh:
        y = model(x.clone())
        return y, y, False
    seen = []
    h = model.outerblock[-2].register_forward_hook(lambda _m, _i, o: seen.append(o.clone()))
    y = model(x.clone())
    h.remove()
    return seen[0], y, True


def main():
    make_golden._install_placeholders()
    sys.path.insert(0, make_golden.REF)
    threads = torch.get_num_threads()
    import mdir                                                     # noqa: F401
    torch.set_num_threads(threads)
    from mdir.components.model.network import unet as ref_unet
    from mdir.components.data import wrapper as ref_wrapper

    T = lambda t: t.detach().cpu().numpy()
    arrays = {"n_cases": np.int64(len(CASES)), "out_channels": np.int64(OUT_CHANNELS)}
    models = []
    with torch.no_grad():
        for i, (label, cls, cfg, shape) in enumerate(CASES):
            model = getattr(ref_unet, cls)(shape[1], OUT_CHANNELS, **cfg).eval()
            model.load_state_dict(case_state(i), strict=True)
            models.append(model)
            p = "c%d_" % i
            arrays[p + "label"] = np.array(label)
            arrays[p + "cfg_names"] = np.array(sorted(cfg))
            arrays[p + "cfg_values"] = np.array([float(cfg[k]) for k in sorted(cfg)], dtype=np.float64)
            arrays[p + "seeds"] = np.array([160 + i, 170 + i], dtype=np.int64)
            arrays[p + "shape"] = np.array(shape, dtype=np.int64)
            arrays[p + "meta_names"] = np.array(sorted(model.meta))
            arrays[p + "meta_values"] = np.array([model.meta[k] for k in sorted(model.meta)], dtype=np.int64)
            arrays[p + "keys"] = np.array(list(model.state_dict().keys()))
            arrays[p + "shapes"] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in model.state_dict().values()], dtype=np.int64)
            x = case_input(i)
            pre, y, tanh = map_and_out(model, x)
            assert tuple(y.shape) == (shape[0], OUT_CHANNELS) + tuple(shape[2:])
            map_max = float(pre.abs().max())
            assert 0.5 <= map_max <= 20.0, (i, map_max)
            arrays[p + "out"] = T(y)
            arrays[p + "has_tanh"] = np.int64(tanh)
            if tanh:
                arrays[p + "pre"] = T(pre)
            arrays[p + "map_max"] = np.float64(map_max)
            emu, _, _ = map_and_out(make_unet_golden.f16_emulation(model), x)
            err = float((emu - pre).abs().max() / pre.abs().max())
            arrays[p + "f16_emulated_err"] = np.float64(err)
            print("case %d %s %s %s: max|map| %.3f  f16_emulated_err %.3e" % (i, label, cfg, shape, map_max, err))
        # ---- the wrapper around an aligned net on a size that its blocks do not divide
        wrap = ref_wrapper.ReflectPadMakeDivisible(WRAP_DIV, "cpu")
        xw = synth.synth_input(WRAP_SEED, WRAP_SHAPE, 1.0)
        padded, padding = wrap.preprocess(xw, None)
        pre, y, _ = map_and_out(models[WRAP_CASE], padded)
        emu, _, _ = map_and_out(make_unet_golden.f16_emulation(models[WRAP_CASE]), padded)
        arrays["wrap_cfg"] = np.array([WRAP_CASE, WRAP_DIV, WRAP_SEED], dtype=np.int64)
        arrays["wrap_shape"] = np.array(WRAP_SHAPE, dtype=np.int64)
        arrays["wrap_padding"] = np.array(padding, dtype=np.int64)
        arrays["wrap_net_out"] = T(wrap.postprocess(y, None, padding))
        arrays["wrap_net_map_max"] = np.float64(float(pre.abs().max()))
        arrays["wrap_net_f16_emulated_err"] = np.float64(float((emu - pre).abs().max() / pre.abs().max()))
        print("wrapper: padding %s; wrapped net max|map| %.3f f16_emulated_err %.3e" % (padding, arrays["wrap_net_map_max"], arrays["wrap_net_f16_emulated_err"]))
    path = os.path.join(HERE, "p2p_unet.npz")
    np.savez_compressed(path, **arrays)
    print("wrote p2p_unet.npz %.1f KiB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
