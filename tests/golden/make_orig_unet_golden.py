"""Generate tests/golden/orig_unet.npz by IMPORTING THE REFERENCE's unet.py (OrigUNet, OutconvP2pUNetDynamicInterpolate) and ReflectPadMakeDivisible
(read-only) -- the way make_p2p_unet_golden.py does.

Runs only where the reference is present.  Weights and inputs are regenerated from seeds on the consumer side (gandtr_amd.tools.synth: ``orig_unet_state`` /
``dynint_unet_state`` filled into the reference module with a strict ``load_state_dict``, so its key list is the reference's).  max|out| of every case lies in
[0.5, 20] (asserted here, stored as ``map_max``).

Stored per case: the label, the constructor arguments (a JSON object), the seeds, the input shape, the key list and shapes, the reference's fp32 output
(``out``), ``flops``: 2 MACs of every Conv2d / ConvTranspose2d of the forward, counted by forward hooks (a transposed conv: every input pixel meets every
kernel tap once), and ``f16_emulated_err``: max|d out| / max|out| of the SAME reference module evaluated on the CPU with every Conv2d / ConvTranspose2d input
and weight rounded to fp16 (fp32 arithmetic otherwise), the BatchNorm behind a conv folded into its weight in fp32 BEFORE the rounding
(make_unet_golden.f16_emulation).  In the dynint nets every F.interpolate result goes straight into a conv, so the emulation rounds it to fp16 as well (the
conv's input rounding) -- as the device does, which stores the resized tensor in fp16.  A figure made of the reference and IEEE rounding alone.

Wrapper record: the reference's ReflectPadMakeDivisible(4) + the net of case 1 (two levels) on a (1, 3, 50, 70) tensor: the cropped output, the range of the
map and the emulation figure of that run.

usage:  python tests/golden/make_orig_unet_golden.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden                                             # noqa: E402  (placeholders, paths)
import make_unet_golden                                        # noqa: E402  (f16_emulation)
from gandtr_amd.tools import synth                             # noqa: E402

# (label, reference class, constructor arguments, input shape); weights seed 260 + i, input seed 270 + i
CASES = (("orig_unet", "OrigUNet", dict(nested_levels=1), (2, 3, 10, 14)),
         ("orig_unet", "OrigUNet", dict(nested_levels=2), (2, 3, 20, 36)),
         ("orig_unet", "OrigUNet", dict(nested_levels=4), (1, 4, 32, 48)),
         ("outconv_dynint_unet", "OutconvP2pUNetDynamicInterpolate", dict(nested_levels=2), (2, 3, 37, 50)),
         ("outconv_dynint_unet", "OutconvP2pUNetDynamicInterpolate", dict(nested_levels=3, batchnorm=True, outconv_kernel=5), (1, 3, 33, 47)),
         ("outconv_dynint_unet", "OutconvP2pUNetDynamicInterpolate", dict(nested_levels=2, upsample="nearest"), (2, 1, 21, 30)),
         ("outconv_dynint_unet", "OutconvP2pUNetDynamicInterpolate", dict(nested_levels=1), (1, 3, 5, 7)))
OUT_CHANNELS = 3
WRAP_CASE, WRAP_DIV, WRAP_SEED, WRAP_SHAPE = 1, 4, 290, (1, 3, 50, 70)


def state_of(label, seed, in_channels, cfg):
    """the synthesised state dict of a net of the fixture (``upsample`` is no parameter of the weights)"""
    if label == "orig_unet":
        return synth.orig_unet_state(seed, in_channels=in_channels, out_channels=OUT_CHANNELS, **cfg)
    return synth.dynint_unet_state(seed, in_channels=in_channels, out_channels=OUT_CHANNELS, **{k: v for k, v in cfg.items() if k != "upsample"})


def case_state(i):
    label, _, cfg, shape = CASES[i]
    return state_of(label, 260 + i, shape[1], cfg)


def case_input(i):
    return synth.synth_input(270 + i, CASES[i][3], 1.0)


def hooked_flops(model, x):
    """(output, 2 MACs of every Conv2d / ConvTranspose2d) of one forward"""
    total = [0.0]

    def hook(mod, args, out):
        k = mod.kernel_size[0] * mod.kernel_size[1]
        px = args[0].shape[0] * args[0].shape[2] * args[0].shape[3] if isinstance(mod, torch.nn.ConvTranspose2d) else out.shape[0] * out.shape[2] * out.shape[3]
        total[0] += 2.0 * px * mod.in_channels * mod.out_channels * k

    hs = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d))]
    y = model(x.clone())
    for h in hs:
        h.remove()
    return y, total[0]


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
            arrays[p + "cfg"] = np.array(json.dumps(cfg, sort_keys=True))
            arrays[p + "seeds"] = np.array([260 + i, 270 + i], dtype=np.int64)
            arrays[p + "shape"] = np.array(shape, dtype=np.int64)
            arrays[p + "meta_names"] = np.array(sorted(model.meta))
            arrays[p + "meta_values"] = np.array([model.meta[k] for k in sorted(model.meta)], dtype=np.int64)
            arrays[p + "keys"] = np.array(list(model.state_dict().keys()))
            arrays[p + "shapes"] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in model.state_dict().values()], dtype=np.int64)
            x = case_input(i)
            y, flops = hooked_flops(model, x)
            assert tuple(y.shape) == (shape[0], OUT_CHANNELS) + tuple(shape[2:])
            map_max = float(y.abs().max())
            assert 0.5 <= map_max <= 20.0, (i, map_max)
            arrays[p + "out"] = T(y)
            arrays[p + "map_max"] = np.float64(map_max)
            arrays[p + "flops"] = np.float64(flops)
            emu = make_unet_golden.f16_emulation(model)(x.clone())
            err = float((emu - y).abs().max() / y.abs().max())
            arrays[p + "f16_emulated_err"] = np.float64(err)
            print("case %d %s %s %s: max|out| %.3f  flops %.4g  f16_emulated_err %.3e" % (i, label, cfg, shape, map_max, flops, err))
        # ---- the wrapper around the two-level net on a size that its pools do not divide
        wrap = ref_wrapper.ReflectPadMakeDivisible(WRAP_DIV, "cpu")
        xw = synth.synth_input(WRAP_SEED, WRAP_SHAPE, 1.0)
        padded, padding = wrap.preprocess(xw, None)
        y = models[WRAP_CASE](padded.clone())
        emu = make_unet_golden.f16_emulation(models[WRAP_CASE])(padded.clone())
        arrays["wrap_cfg"] = np.array([WRAP_CASE, WRAP_DIV, WRAP_SEED], dtype=np.int64)
        arrays["wrap_shape"] = np.array(WRAP_SHAPE, dtype=np.int64)
        arrays["wrap_padding"] = np.array(padding, dtype=np.int64)
        arrays["wrap_net_out"] = T(wrap.postprocess(y, None, padding))
        arrays["wrap_net_map_max"] = np.float64(float(y.abs().max()))
        arrays["wrap_net_f16_emulated_err"] = np.float64(float((emu - y).abs().max() / y.abs().max()))
        print("wrapper: padding %s; wrapped net max|out| %.3f f16_emulated_err %.3e" % (padding, arrays["wrap_net_map_max"], arrays["wrap_net_f16_emulated_err"]))
    path = os.path.join(HERE, "orig_unet.npz")
    np.savez_compressed(path, **arrays)
    print("wrote orig_unet.npz %.1f KiB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
