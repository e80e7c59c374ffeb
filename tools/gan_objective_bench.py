"""dev tool: the GAN scenarios' objectives on one device (gandtr_amd/csrc/map_loss.hip, gandtr_amd/learning/epoch_iteration), synthetic weights.  Everything
is compared inside this process, alternating, after a warm-up of every variant:
  (a) gdt_map_loss alone at 64 x 3 x 256^2 (one l1 pair: 100 MB read) and at 64 x 1 x 256^2 with the sigmoid flag -- through the C ABI with preallocated
      buffers, through ``L1Loss()(a, b)`` / ``map_losses`` (allocations included) -- against ``torch.nn.functional.l1_loss`` on the same tensors, and the
      achieved bytes/s against the 6.29 TB/s of a float4 copy on this chip;
  (b) ``step_losses`` of HED-N-GAN (BatchNorm generator and discriminator, the scenario's) and of CycleGAN (InstanceNorm) at 16 x 3 x 256^2 against the same
      terms composed naively from this repository's own modules: one forward per call of the reference's ``_optimization_step`` (ten each) and torch ops for
      the terms.
Each timed sample is a burst of calls between two events divided by the burst length.  Event-timed bursts run at higher clocks than a sustained run: they
rank variants; bench.py quotes speed.  Prints one JSON line and writes it to the path given (default profiles/gan_objective_1gpu.json).
With ``--data DIR`` the inputs of (b) are one batch of the scenarios' own training data instead of synthetic tensors: DIR/train_day.txt and DIR/train_night.txt
(one file name per line) over the images in DIR/ims, read through the ``train`` block of parameters/_gan_data.yml (RandomDomainsPair,
``pil2np | scalecrop:256_256:0.8_1 | totensor | normalize``) by gandtr_amd.components.data.dataset.initialize_dataset_loader -- decode, crop and resize on the device.
usage: tools/gan_objective_bench.py [iters] [out.json] [--data DIR]      (default 10 timed bursts per variant)"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                     # noqa: E402
import torch.nn.functional as F                                  # noqa: E402

from gandtr_amd import _hip                                      # noqa: E402
from gandtr_amd.components.model.network import hed, p2p_networks     # noqa: E402
from gandtr_amd.components.optim.criterion import compound       # noqa: E402
from gandtr_amd.learning import epoch_iteration                  # noqa: E402
from gandtr_amd.tools import synth                               # noqa: E402

data_dir = None
if "--data" in sys.argv:
    at = sys.argv.index("--data")
    data_dir = sys.argv[at + 1]
    del sys.argv[at:at + 2]
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 10
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gan_objective_1gpu.json")
dev = torch.device("cuda:0")
COPY_RATE = 6.29e12                                              # float4 copy, bytes/s
KERNEL_BURST, STEP_BURST = 50, 2


def timed(fn, burst):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(burst):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / burst


def stats(v):
    v = sorted(v)
    return {"ms_median": round(v[len(v) // 2], 5), "ms_min": round(v[0], 5), "ms_max": round(v[-1], 5)}


def alternate(variants, burst):
    vals = {k: float(fn()) for k, fn in variants.items()}         # warm-up of every variant, and their values
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(iters):
        for k, fn in variants.items():
            t[k].append(timed(fn, burst))
    row = {k: stats(v) for k, v in t.items()}
    row["values"] = {k: round(v, 6) for k, v in vals.items()}
    return row


def kernel_rows():
    lib = _hip.load()
    rows = {}
    for name, shape, sigmoid in (("l1_64x3x256x256", (64, 3, 256, 256), False), ("l1_sigmoid_64x1x256x256", (64, 1, 256, 256), True)):
        a, b = synth._normal(1, "bench.a", shape).to(dev), synth._normal(1, "bench.b", shape).to(dev)
        table = (_hip.MapLossPair * 1)(_hip.MapLossPair(a.data_ptr(), b.data_ptr(), 0.0, 0, 1 if sigmoid else 0, shape[0], a.numel(), 1.0))
        nbytes = ctypes.c_size_t()
        _hip.check(lib.gdt_map_loss_workspace_bytes(table, 1, ctypes.byref(nbytes)))
        ws = torch.empty(nbytes.value // 8, dtype=torch.float64, device=dev)
        out = torch.empty(shape[0] + 2, dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def c_abi():
            _hip.check(lib.gdt_map_loss(table, 1, out.data_ptr(), out[shape[0]:].data_ptr(), out[shape[0] + 1:].data_ptr(), ws.data_ptr(), nbytes.value, stream))
            return out[shape[0]]

        crit = compound.L1Loss()
        variants = {"c_abi": c_abi,
                    "criterion": (lambda: compound.map_losses([crit.pairs(a, b, sigmoid=True)]).per_pair[0]) if sigmoid else (lambda: crit(a, b)),
                    "torch_l1_loss": (lambda: F.l1_loss(torch.sigmoid(a), torch.sigmoid(b))) if sigmoid else (lambda: F.l1_loss(a, b))}
        row = alternate(variants, KERNEL_BURST)
        nbytes_read = 2 * a.numel() * 4
        row["bytes_read"] = nbytes_read
        for k in ("c_abi", "criterion"):
            row[k]["bytes_per_s"] = round(nbytes_read / (row[k]["ms_median"] * 1e-3), 0)
            row[k]["share_of_float4_copy_rate"] = round(row[k]["bytes_per_s"] / COPY_RATE, 3)
        row["torch_over_c_abi"] = round(row["torch_l1_loss"]["ms_median"] / row["c_abi"]["ms_median"], 2)
        row["torch_over_criterion"] = round(row["torch_l1_loss"]["ms_median"] / row["criterion"]["ms_median"], 2)
        rows[name] = row
    return rows


def module(cls, state, *args, **kwargs):
    net = cls(*args, **kwargs).eval()
    net.load_state_dict(state)
    return net.to(dev)


def mse_const(pred, target):
    return F.mse_loss(pred, torch.full(pred.shape, float(target), dtype=torch.float32, device=pred.device))


def naive_hedngan(nets, weights, X, Y):
    """edges_epochs.py:61-121 forward by forward: ten graph runs, torch ops for the terms"""
    G, D, S, T = nets["generator_X"], nets["discriminator_Y"], nets["detector"], nets["detector_frozen"]
    fake_Y = G(X)
    D_real, D_fake = weights["adversarial"] * mse_const(D(Y), 0), weights["adversarial"] * mse_const(D(fake_Y), 1)
    target_M = T(X, no_sigmoid=True)
    E_real = weights["hed"] * F.l1_loss(S(X, no_sigmoid=True), target_M)
    E_fake = weights["hed"] * F.l1_loss(S(fake_Y, no_sigmoid=True), target_M)
    fake_E, real_E, _check = S(fake_Y), T(X), S(X)
    G_gan = weights["adversarial"] * mse_const(D(fake_Y), 0)
    G_hed = weights["edge"] * F.l1_loss(fake_E, real_E)
    return G_gan + G_hed + (D_real + D_fake) * 0.5, E_real, E_fake


def naive_cyclegan(nets, X, Y):
    """gan_epochs.py:68-140 forward by forward: ten graph runs, torch ops for the terms"""
    G_X, G_Y, D_X, D_Y = nets["generator_X"], nets["generator_Y"], nets["discriminator_X"], nets["discriminator_Y"]
    fake_Y = G_X(X)
    rec_X = G_Y(fake_Y)
    fake_X = G_Y(Y)
    rec_Y = G_X(fake_X)
    loss_G_X = mse_const(D_X(fake_Y), 0) + 10 * F.l1_loss(rec_X, X)
    loss_G_Y = mse_const(D_Y(fake_X), 0) + 10 * F.l1_loss(rec_Y, Y)
    loss_D_X = (mse_const(D_X(Y), 0) + mse_const(D_X(fake_Y), 1)) * 0.5
    loss_D_Y = (mse_const(D_Y(X), 0) + mse_const(D_Y(fake_X), 1)) * 0.5
    return loss_G_X + loss_G_Y + loss_D_X + loss_D_Y


def data_batch(root, batch_size):
    """one batch of parameters/_gan_data.yml's ``train`` block over the lists and images under ``root``"""
    import random
    import numpy as np
    from gandtr_amd.components.data import dataset
    params = {"dataset": {"name": "RandomDomainsPair", "dataset_X": os.path.join(root, "train_day.txt"), "dataset_Y": os.path.join(root, "train_night.txt"),
                          "image_dir": os.path.join(root, "ims") + "/*", "size": batch_size},
              "loader": {"batch_size": batch_size}, "transforms": "pil2np | scalecrop:256_256:0.8_1 | totensor | normalize",
              "mean_std": [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]]}
    loader = dataset.initialize_dataset_loader(None, "train", params, device=dev)
    np.random.seed(0)
    random.seed(0)
    loader.dataset.prepare_epoch(None, None)
    return next(iter(loader))


def step_rows():
    shape = (16, 3, 256, 256)
    if data_dir is not None:
        X, Y = data_batch(data_dir, shape[0])
    else:
        X, Y = synth.synth_input(2, shape, 1.0, name="src").to(dev), synth.synth_input(2, shape, 1.0, name="tgt").to(dev)
    rows = {}
    adv = {"loss": "discriminator_loss", "criterion": {"loss": "mse"}}
    weights = {"adversarial": 1, "edge": 5, "hed": 1}
    nets = {"generator_X": module(p2p_networks.ResnetGenerator, synth.generator_state(0, "batch"), 3, 3, norm_layer="batch"),
            "discriminator_Y": module(p2p_networks.NLayerDiscriminator, synth.discriminator_state(41, "batch", gain=0.2), 3, norm_layer="batch"),
            "detector": module(hed.HedInterpolation, synth.hed_state(5)), "detector_frozen": module(hed.HedInterpolation, synth.hed_state(0))}
    epoch = epoch_iteration.EPOCH_ITERATIONS["SupervisedHEDNGANEpoch"](compound.initialize_gan_criterion(
        {"loss": "multihead_loss", "weights": weights, "normalize_weights": False, "adversarial": adv, "edge": {"loss": "l1"}, "hed": {"loss": "l1"}}))
    row = alternate({"step_losses": lambda: epoch.step_losses(nets, X, Y)[0]["total"], "naive": lambda: naive_hedngan(nets, weights, X, Y)[0]}, STEP_BURST)
    row["graph_runs"] = {"step_losses": 4, "naive": 10}
    row["naive_over_step_losses"] = round(row["naive"]["ms_median"] / row["step_losses"]["ms_median"], 3)
    rows["hedngan_16x3x256x256"] = row
    g = {"loss": "multihead_loss", "weights": {"adversarial": 1, "cycle": 10}, "normalize_weights": False, "adversarial": {"loss": "mse"}, "cycle": {"loss": "l1"}}
    nets = {"generator_X": module(p2p_networks.ResnetGenerator, synth.generator_state(0, "instance"), 3, 3, norm_layer="instance"),
            "generator_Y": module(p2p_networks.ResnetGenerator, synth.generator_state(1, "instance"), 3, 3, norm_layer="instance"),
            "discriminator_X": module(p2p_networks.NLayerDiscriminator, synth.discriminator_state(40, "instance", gain=0.2), 3, norm_layer="instance"),
            "discriminator_Y": module(p2p_networks.NLayerDiscriminator, synth.discriminator_state(41, "instance", gain=0.2), 3, norm_layer="instance")}
    epoch = epoch_iteration.EPOCH_ITERATIONS["SupervisedCycleGanEpoch"](compound.initialize_gan_criterion(
        {"loss": "cycle_loss", "loss_G_X": g, "loss_G_Y": g, "loss_D_X": adv, "loss_D_Y": adv}))
    row = alternate({"step_losses": lambda: epoch.step_losses(nets, X, Y)[0]["total"], "naive": lambda: naive_cyclegan(nets, X, Y)}, STEP_BURST)
    row["graph_runs"] = {"step_losses": 6, "naive": 10}
    row["naive_over_step_losses"] = round(row["naive"]["ms_median"] / row["step_losses"]["ms_median"], 3)
    rows["cyclegan_16x3x256x256"] = row
    return rows


out = {"workload": "gdt_map_loss and the GAN scenarios' step_losses, synthetic weights, generator f16c, discriminator / HED f16",
       "inputs": "synthetic" if data_dir is None else "RandomDomainsPair over " + data_dir, "iters": iters, "kernel_burst": KERNEL_BURST, "step_burst": STEP_BURST, "float4_copy_rate_bytes_per_s": COPY_RATE}
with torch.no_grad():
    out["map_loss"] = kernel_rows()
    out["step_losses"] = step_rows()
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
