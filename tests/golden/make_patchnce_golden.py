"""Generate tests/golden/patchnce.npz by IMPORTING THE REFERENCE's PatchSampleF, MultilayerPatchNCELoss and ResnetGenerator (read-only) -- the way
make_discriminator_golden.py does.

Runs only where the reference is present.  Weights and inputs are regenerated from seeds on the consumer side (gandtr_amd.tools.synth:
``patchsample_state`` filled into the reference module with a strict ``load_state_dict``, ``patchnce_maps``, ``generator_state``, ``synth_input``).  The
reference's PatchSampleF is built with ``input_nc=None, nce_layers=None`` and ``create_mlp(feats, "cpu")``: its default constructor path calls ``.cuda()``.

Head cases ``h<i>_`` (synthetic fp32 maps): shape (B, C, H, W, P, nc; nc 0 = use_mlp off), the ids drawn under ``np.random.seed``, the reference's pooled
rows of both sides, and for ``batch_dim_for_bmm`` 1 and B the per-row losses, the layer mean and the total.  The head cases run the reference's modules in
FLOAT64 (``.double()`` modules on the fp32 maps and weights widened exactly): an fp32 run of the same ops carries its own error of up to 6e-6 in a row loss
(1 / T = 14 times the rounding of a 256-term dot product), which depends on the BLAS code path of the machine that wrote the file; the float64 values
are what every fp32 evaluation -- the mirror's CPU path on any machine, the device -- is within its derived bound of.  Row losses, means and totals
are stored as float64, the pooled rows rounded to fp32 (unit rows: 6e-8).  Checked here: no pooled row has a pre-normalisation norm below 1e-3 (the
``+ 1e-7`` of Normalize stays a detail).

Pipeline cases ``p<i>_`` (the 9-block InstanceNorm generator, layers 4,8,12,16): the ids, the per-row losses, layer means and total of the forward of
``SupervisedCutEpoch.calculate_nce_loss`` (cut_epochs.py:79-89) and ``f16_emulated_row_err``: per layer, max over rows of |row loss (fp32 reference) - row
loss (the SAME reference with every generator conv weight and conv input rounded to fp16)| -- a figure made of the reference and IEEE rounding alone.

usage:  python tests/golden/make_patchnce_golden.py
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

TEMPERATURE, WEIGHT = 0.07, 1.0
# (B, C, H, W, P, nc): nc 0 = use_mlp off; weights seed 60 + i, maps seed 70 + i, ids seed 80 + i
HEAD_CASES = ((3, 128, 9, 13, 37, 256), (2, 256, 6, 7, 64, 256), (2, 24, 5, 5, 16, 40), (1, 256, 8, 8, 64, 256), (2, 128, 9, 13, 37, 0))
# (input shape); generator seed 0 (gain 0.02), featdown seed 90, inputs seed 91 + i / name src|tgt, ids seed 95 + i
NCE_LAYERS = "4,8,12,16"
PIPE_CASES = ((2, 3, 40, 52), (1, 3, 24, 28))
PIPE_PATCHES = 64


def f16_emulation(model):
    """a copy of ``model`` whose convs see fp16-rounded weights and fp16-rounded inputs (fp32 arithmetic otherwise)"""
    m = copy.deepcopy(model)
    for mod in m.modules():
        if isinstance(mod, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
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
    arrays = {"n_head_cases": np.int64(len(HEAD_CASES)), "n_pipe_cases": np.int64(len(PIPE_CASES)), "temperature": np.float64(TEMPERATURE),
              "weight": np.float64(WEIGHT), "nce_layers": np.array(NCE_LAYERS), "pipe_patches": np.int64(PIPE_PATCHES)}

    def featdown(feats, use_mlp, nc, seed):
        netF = ref_p2p.PatchSampleF(use_mlp=use_mlp, input_nc=None, nc=nc, nce_layers=None)
        if use_mlp:
            netF.create_mlp(feats, "cpu")
            netF.load_state_dict(synth.patchsample_state(seed, [f.shape[1] for f in feats], nc))
        return netF.eval()

    def losses(q_pool, k_pool, layers, groups, p, arrays):
        crit = ref_losses.MultilayerPatchNCELoss(groups, layers, 0, TEMPERATURE, WEIGHT)
        out = crit(q_pool, k_pool)
        rows = [c(q, k) for c, q, k in zip(crit.losses, q_pool, k_pool)]
        arrays[p + "keys"] = np.array(list(out.partial.keys()))
        dtype = np.float64 if rows[0].dtype == torch.float64 else np.float32
        arrays[p + "means"] = np.array([float(v) for v in out.partial.values()], dtype=dtype)
        arrays[p + "total"] = dtype(float(out.total))
        for l, r in enumerate(rows):
            arrays[p + "rows%d" % l] = T(r)
        return rows

    with torch.no_grad():
        for i, (B, C, H, W, P, nc) in enumerate(HEAD_CASES):
            p = "h%d_" % i
            qmap, kmap = (m.double() for m in synth.patchnce_maps(70 + i, (B, C, H, W)))
            netF = featdown([kmap], nc > 0, nc or 256, 60 + i).double()
            np.random.seed(80 + i)
            k_pool, ids = netF([kmap], num_patches=P, patch_ids=None)
            q_pool, _ = netF([qmap], num_patches=P, patch_ids=ids)
            raw = kmap.permute(0, 2, 3, 1).flatten(1, 2)[:, ids[0], :].flatten(0, 1)
            raw_q = qmap.permute(0, 2, 3, 1).flatten(1, 2)[:, ids[0], :].flatten(0, 1)
            pre = [netF.mlp_0(r) if nc else r for r in (raw, raw_q)]
            min_norm = min(float(x.norm(dim=1).min()) for x in pre)
            assert min_norm > 1e-3, min_norm
            arrays[p + "shape"] = np.array([B, C, H, W, P, nc], dtype=np.int64)
            arrays[p + "ids"] = T(ids[0]).astype(np.int32)
            arrays[p + "q"] = T(q_pool[0]).astype(np.float32)
            arrays[p + "k"] = T(k_pool[0]).astype(np.float32)
            if nc:
                arrays[p + "keys"] = np.array(list(netF.state_dict().keys()))
                arrays[p + "shapes"] = np.array([list(v.shape) + [0] * (2 - v.dim()) for v in netF.state_dict().values()], dtype=np.int64)
            spread = []
            for groups in (1, B):
                rows = losses(q_pool, k_pool, "0", groups, p + "g%d_" % groups, arrays)
                spread.append((float(rows[0].min()), float(rows[0].max())))
            print("head case %d %s: %d rows, min pre-norm %.3f, row loss range %s" % (i, (B, C, H, W, P, nc), q_pool[0].shape[0], min_norm, spread))

        netG = ref_p2p.ResnetGenerator(3, 3, norm_layer="instance").eval()
        netG.load_state_dict(synth.generator_state(0, "instance"))
        emuG = f16_emulation(netG)
        layers = [int(v) for v in NCE_LAYERS.split(",")]
        for i, shape in enumerate(PIPE_CASES):
            p = "p%d_" % i
            src, tgt = synth.synth_input(91 + i, shape, 1.0, name="src"), synth.synth_input(91 + i, shape, 1.0, name="tgt")
            # calculate_nce_loss(output=src, target=tgt): q from the target, k from the output

            def run(net, ids):
                feat_q = net.forward(tgt, layers=list(layers), encode_only=True)
                feat_k = net.forward(src, layers=list(layers), encode_only=True)
                netF = featdown(feat_k, True, 256, 90)
                feat_k_pool, sample_ids = netF(feat_k, num_patches=PIPE_PATCHES, patch_ids=ids)
                feat_q_pool, _ = netF(feat_q, num_patches=PIPE_PATCHES, patch_ids=sample_ids)
                return feat_q_pool, feat_k_pool, sample_ids

            np.random.seed(95 + i)
            q_pool, k_pool, ids = run(netG, None)
            arrays[p + "shape"] = np.array(shape, dtype=np.int64)
            for l, t in enumerate(ids):
                arrays[p + "ids%d" % l] = T(t).astype(np.int32)
            B = shape[0]
            for groups in sorted({1, B}):
                rows = losses(q_pool, k_pool, NCE_LAYERS, groups, p + "g%d_" % groups, arrays)
                eq, ek, _ = run(emuG, ids)
                crit = ref_losses.MultilayerPatchNCELoss(groups, NCE_LAYERS, 0, TEMPERATURE, WEIGHT)
                emu = [c(q, k) for c, q, k in zip(crit.losses, eq, ek)]
                err = np.array([float((a - b).abs().max()) for a, b in zip(rows, emu)])
                arrays[p + "g%d_f16_emulated_row_err" % groups] = err
                print("pipeline case %d %s groups %d: rows %s, total %.4f, row loss range %.3f .. %.3f, f16_emulated_row_err %s" %
                      (i, shape, groups, [int(r.numel()) for r in rows], float(arrays[p + "g%d_total" % groups]),
                       min(float(r.min()) for r in rows), max(float(r.max()) for r in rows), err))
    path = os.path.join(HERE, "patchnce.npz")
    np.savez_compressed(path, **arrays)
    print("wrote patchnce.npz %.1f KiB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
