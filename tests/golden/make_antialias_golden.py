"""Generate the fixtures of the anti-aliased ResnetGenerator (CUT's defaults: no_antialias=False / no_antialias_up=False) by running the REFERENCE's module.

The reference's mdir/components/model/network/p2p_networks.py imports on its own (numpy, torch), so it is loaded by path; the weights come from
gandtr_amd.tools.synth.generator_state with the two flags, the inputs from synth.synth_input, and only results are stored:

  gen_tiny_aa_instance.npz / gen_tiny_aa_batch.npz   ngf 8, 2 blocks, both flags off, on synth_input(1, (2, 3, 32, 32), 1.0): the output and every tap
  gen_tiny_aa_cases.npz                              mixed flags (Downsample + ConvTranspose2d; stride-2 convs + Upsample) on the same input, and both flags off on the
                                                     odd size synth_input(1, (1, 3, 21, 18), 1.0) (output 24 x 20): the output and the taps a device can deliver

What "every tap" is in a file: ``layers`` = the number of nn.Sequential entries; ``tap<i>`` for every index whose tensor is not, bit for bit, one already stored;
``same_as`` [layers]: the index whose array holds tap i (i itself when stored) -- the reference's ReLUs are in place, so a norm layer's tap IS the ReLU's -- or -1 for
the two reflection-padded tensors (index 0 and the pad in front of the head), which are F.pad(.., (3, 3, 3, 3), "reflect") of the input / of the previous tap (asserted
here) and are not stored.  ``images`` [layers]: how many images of the batch ``tap<i>`` holds -- all of them, but for the widest full-resolution maps (more than
100 KiB for the batch: the 16-channel 32 x 32 tensors), which hold image 0 only; every layer treats the images of a batch independently in eval mode, and image 1 of
those maps is what the next stored tap is computed from.  ``out`` is the last tap.  That keeps every file under the size of the largest fixture of this directory.

usage:  python tests/golden/make_antialias_golden.py <root of the reference checkout>
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from gandtr_amd.tools import synth                            # noqa: E402

LIMIT = 700 * 1024


def load_reference(root):
    path = os.path.join(root, "mdir", "components", "model", "network", "p2p_networks.py")
    spec = importlib.util.spec_from_file_location("reference_p2p_networks", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(ref, norm, x, no_antialias, no_antialias_up, ngf=8, n_blocks=2):
    """{"layers", "same_as", "images", "tap<i>"} of the reference generator on ``x`` (see the module docstring)"""
    g = ref.ResnetGenerator(3, 3, ngf=ngf, norm_layer=norm, n_blocks=n_blocks, no_antialias=no_antialias, no_antialias_up=no_antialias_up).eval()
    g.load_state_dict(synth.generator_state(0, norm, ngf=ngf, n_blocks=n_blocks, no_antialias=no_antialias, no_antialias_up=no_antialias_up), strict=True)
    layers = len(g.model)
    with torch.no_grad():
        out, feats = g(x, layers=list(range(layers)))
    assert len(feats) == layers and torch.equal(out, feats[-1])
    arrays, same_as, images = {}, [], []
    for i, f in enumerate(feats):
        if i in (0, layers - 3):                     # the two reflection pads
            assert torch.equal(f, F.pad(x if i == 0 else feats[i - 1], (3, 3, 3, 3), mode="reflect"))
            same_as.append(-1)
            images.append(0)
            continue
        j = next((k for k in range(i) if same_as[k] == k and feats[k].shape == f.shape and torch.equal(feats[k], f)), i)
        same_as.append(j)
        images.append(1 if f.numel() * 4 > 100 * 1024 else f.shape[0])
        if j == i:
            arrays["tap%d" % i] = f[:images[-1]].numpy()
    arrays["layers"] = np.int64(layers)
    arrays["same_as"] = np.asarray(same_as, dtype=np.int64)
    arrays["images"] = np.asarray(images, dtype=np.int64)
    return arrays


def save(name, arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print("wrote %-28s %7.1f KiB" % (name + ".npz", size / 1024))
    assert size <= LIMIT, (name, size)


def main(root):
    ref = load_reference(root)
    x = synth.synth_input(1, (2, 3, 32, 32), 1.0)
    for norm in ("instance", "batch"):
        save("gen_tiny_aa_" + norm, run(ref, norm, x, False, False))
    cases = {}
    odd = synth.synth_input(1, (1, 3, 21, 18), 1.0)
    for tag, (xin, aa, aau) in {"down": (x, False, True), "up": (x, True, False), "odd": (odd, False, False)}.items():
        r = run(ref, "instance", xin, aa, aau)
        if tag != "odd":                             # the mixed cases keep the output and the taps around their sampling layers: the rest is the layout test's
            layers = int(r["layers"])
            keep = {"layers", "same_as", "images", "tap%d" % (layers - 1)} | {"tap%d" % r["same_as"][i] for i in ((4, 6, 7, 10, 11) if tag == "down" else (12, 13, 15, 16, 17, 19))}
            r["same_as"] = np.asarray([s if s < 0 or "tap%d" % s in keep else -2 for s in r["same_as"]], dtype=np.int64)      # -2: not stored in this file
            r = {k: v for k, v in r.items() if k in keep}
            assert layers == 23
        cases.update({"%s_%s" % (tag, k): v for k, v in r.items()})
    save("gen_tiny_aa_cases", cases)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
