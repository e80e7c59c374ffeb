"""dev tool: CUT's contrastive head (PatchSampleF + MultilayerPatchNCELoss, gandtr_amd/csrc/patch_nce.hip) on one device, synthetic weights.  Everything is
compared inside this process, alternating, after a warm-up of every variant:
  * the fused head (three launches) against the reference's op sequence written with torch ops on the same GPU (per layer and side: permute, gather, two
    addmm, relu, the norm; per layer: two bmm, eye, masked_fill, cat, div, cross entropy, mean), at the scenario's shape -- B = 1, maps 128 x 128^2 and
    three times 256 x 64^2, P = 256, T = 0.07, batch_dim_for_bmm 1 -- and at B = 16 with batch_dim_for_bmm 1 and 16; both take the same device-side ids;
  * calculate_nce_loss as a whole on 256^2 images (9-block InstanceNorm generator, f16c) with the encoder-only graph and with the full graph.
Each timed sample is a burst of calls between two events (a single call is a few launches: shorter than the event resolution is honest about), divided by
the burst length.  Event-timed bursts run at higher clocks than a sustained run: they rank variants; bench.py quotes speed.
Prints one JSON line and writes it to the path given (default profiles/patchnce_1gpu.json).
usage: tools/patchnce_bench.py [iters] [out.json]      (default 20 timed bursts per variant)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                # noqa: E402
import torch                                                     # noqa: E402

from gandtr_amd.components.model.network import p2p_networks     # noqa: E402
from gandtr_amd.components.optim.criterion import patchnce       # noqa: E402
from gandtr_amd.tools import synth                               # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "patchnce_1gpu.json")
dev = torch.device("cuda:0")
T, P, NC = 0.07, 256, 256
MAPS = ((128, 128, 128), (256, 64, 64), (256, 64, 64), (256, 64, 64))          # (C, H, W) of the taps 4, 8, 12, 16 of a 256^2 image
BURST = 10

netF = p2p_networks.PatchSampleF(input_nc=3, nc=NC, nce_layers="4,8,12,16").eval()
netF.load_state_dict(synth.patchsample_state(0, [m[0] for m in MAPS], NC))
netF = netF.to(dev)


def timed(fn, burst=BURST):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(burst):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / burst


def stats(v):
    v = sorted(v)
    return {"ms_median": round(v[len(v) // 2], 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4)}


def torch_head(feats_q, feats_k, ids, groups):
    """the reference's op sequence (p2p_networks.py:641-671, compound_losses.py:127-173) on device tensors, ids given"""
    pools = []
    for feats in (feats_k, feats_q):
        pool = []
        for l, feat in enumerate(feats):
            x = feat.permute(0, 2, 3, 1).flatten(1, 2)[:, ids[l], :].flatten(0, 1)
            x = getattr(netF, "mlp_%d" % l)(x)
            pool.append(x.div(x.pow(2).sum(1, keepdim=True).pow(0.5) + 1e-7))
        pools.append(pool)
    total = 0.0
    for q, k in zip(pools[1], pools[0]):
        n, d = q.shape
        l_pos = torch.bmm(q.view(n, 1, -1), k.view(n, -1, 1)).view(n, 1)
        qg, kg = q.view(groups, -1, d), k.view(groups, -1, d)
        l_neg = torch.bmm(qg, kg.transpose(2, 1))
        l_neg.masked_fill_(torch.eye(qg.size(1), device=dev, dtype=torch.bool)[None, :, :], -10.0)
        out = torch.cat((l_pos, l_neg.view(-1, qg.size(1))), dim=1) / T
        loss = torch.nn.functional.cross_entropy(out, torch.zeros(n, dtype=torch.long, device=dev), reduction="none")
        total = total + torch.mean(loss * 1.0)
    return total / len(feats_q)


def fused_head(feats_q, feats_k, ids, crit):
    k_pool, _ = netF(feats_k, num_patches=P, patch_ids=ids)
    q_pool, _ = netF(feats_q, num_patches=P, patch_ids=ids)
    return crit(q_pool, k_pool).total


def fused_head_one_batch(feats_qk, ids, crit):
    """how calculate_nce_loss calls it: both sides as one batch, one sampling launch"""
    pooled, _ = netF(feats_qk, num_patches=P, patch_ids=ids)
    return crit([p[:p.shape[0] // 2] for p in pooled], [p[p.shape[0] // 2:] for p in pooled]).total


def head_flops_bytes(B, groups):
    """algorithmic operations of the head (two sides) and the bytes it must move: gathered elements (one 64-byte sector each at least), weights once, rows out and in"""
    rows = B * P
    fl = sum(2 * 2 * rows * (c * NC + NC * NC) for c, _, _ in MAPS) + len(MAPS) * (2 * rows * (rows // groups) * NC + 2 * rows * NC)
    by = sum(2 * rows * c * 64 + 4 * (c * NC + NC * NC + 2 * NC) + 2 * 2 * rows * NC * 4 for c, _, _ in MAPS)
    return fl, by


out = {"workload": "PatchSampleF(nc 256) + MultilayerPatchNCELoss(T 0.07), 4 layers, maps 128x128^2 + 3 x 256x64^2, P 256, fp32, synthetic weights",
       "iters": iters, "burst": BURST, "head": {}}
with torch.no_grad():
    for B, groups in ((1, 1), (16, 1), (16, 16)):
        fq = [synth.patchnce_maps(10 + l, (B,) + m)[0].to(dev) for l, m in enumerate(MAPS)]
        fk = [synth.patchnce_maps(10 + l, (B,) + m)[1].to(dev) for l, m in enumerate(MAPS)]
        fqk = [torch.cat([a, b]) for a, b in zip(fq, fk)]
        np.random.seed(B)
        ids = [torch.from_numpy(np.random.permutation(h * w)[:P]).to(dev) for _, h, w in MAPS]
        crit = patchnce.MultilayerPatchNCELoss(groups, "4,8,12,16", P, T, 1.0)
        variants = {"fused": lambda: fused_head(fq, fk, ids, crit), "fused_one_batch": lambda: fused_head_one_batch(fqk, ids, crit),
                    "torch_ops": lambda: torch_head(fq, fk, ids, groups)}
        vals = {k: float(fn()) for k, fn in variants.items()}                 # warm-up of every variant, and the three agree
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in variants}
        for _ in range(iters):
            for k, fn in variants.items():
                t[k].append(timed(fn))
        fl, by = head_flops_bytes(B, groups)
        row = {k: stats(v) for k, v in t.items()}
        row["loss_values"] = {k: round(v, 6) for k, v in vals.items()}
        row["torch_over_fused"] = round(row["torch_ops"]["ms_median"] / row["fused"]["ms_median"], 2)
        row["torch_over_fused_one_batch"] = round(row["torch_ops"]["ms_median"] / row["fused_one_batch"]["ms_median"], 2)
        row["gflop"] = round(fl / 1e9, 3)
        row["floor_ms_fp32_157tflops"] = round(fl / 157.3e12 * 1e3, 4)
        row["floor_ms_traffic_8tbs"] = round(by / 8e12 * 1e3, 4)
        row["fused_launches"] = {"fused": 4, "fused_one_batch": 3}
        out["head"]["B%d_groups%d" % (B, groups)] = row

    # the whole of calculate_nce_loss at the scenario's operating point: 256^2 images, batch 1 and 16, with and without the encoder-only graph
    netG = p2p_networks.ResnetGenerator(3, 3, norm_layer="instance").eval()
    netG.load_state_dict(synth.generator_state(0, "instance"))
    netG = netG.to(dev)
    out["calculate_nce_loss"] = {}
    for B in (1, 16):
        src, tgt = synth.synth_input(20, (B, 3, 256, 256), 1.0).to(dev), synth.synth_input(21, (B, 3, 256, 256), 1.0).to(dev)
        np.random.seed(B)
        ids = [torch.from_numpy(np.random.permutation(h * w)[:P]).to(dev) for _, h, w in MAPS]
        crit = patchnce.MultilayerPatchNCELoss(1, "4,8,12,16", P, T, 1.0)

        def whole(encoder_graph):
            netG.hip_encoder_graph = encoder_graph
            return patchnce.calculate_nce_loss(crit, netG, netF, src, tgt, patch_ids=ids).total

        vals = {str(g): float(whole(g)) for g in (True, False)}
        for g in (True, False):
            for _ in range(3):
                whole(g)
        torch.cuda.synchronize()
        t = {True: [], False: []}
        for _ in range(iters):
            for g in (True, False):
                t[g].append(timed(lambda: whole(g), burst=4))
        row = {"encoder_only_graph": stats(t[True]), "full_graph": stats(t[False]), "loss_values": vals}
        row["full_over_encoder_only"] = round(row["full_graph"]["ms_median"] / row["encoder_only_graph"]["ms_median"], 3)
        out["calculate_nce_loss"]["B%d" % B] = row
    netG.hip_encoder_graph = True
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
