"""Generate tests/golden/gan_objective.npz by IMPORTING THE REFERENCE's criteria and epoch iterations (read-only) -- the way make_patchnce_golden.py does.

Runs only where the reference is present.  Weights and inputs are regenerated from seeds on the consumer side (tests/gan_objective_fixture.py over
gandtr_amd.tools.synth); the file holds scalars, ids and error figures only.

Criterion cases: the reference's ``L1Loss`` / ``MSELoss`` (``c<i>_``), ``MultiheadLoss`` (``m<i>_``) and ``CombinationLoss`` (``k<i>_``) run in FLOAT64 on
fp32 maps of awkward shapes widened exactly, dict / scalar / normalised weights.

Step cases (``<name>_``): the dict the reference's ``_optimization_step`` logs -- keys in order, values from fp32 networks (``f32``) and from ``.double()``
networks on the widened inputs (``f64``) -- with every optimizer a no-op and every network in ``.eval()``.  The epoch object is made with ``__new__`` and
given its criterion (and empty image pools), the optimizers are stubs, the networks sit in a small object's ``.networks`` dict, CycleGAN's discriminators
and CUT's featdown behind a holder with ``.model``.  ``emu_<map>``: max |map - map of the same networks with every conv weight and conv input rounded to
fp16| for every map a term reads (the post-sigmoid maps of the edge term as ``sig_*``); CUT: the two id sets and ``f16_emulated_row_err`` per layer for
both patch-NCE terms (make_patchnce_golden.py), with the emulation applied to the generator that also produced the translation.

The script asserts what keeps the device gate from being vacuous: losses that a wiring mistake would exchange differ by more than the sum of their gates
(all cases but ``cyclegan_plain``, which exists to run both generators with ordinary weights).

usage:  python tests/golden/make_gan_objective_golden.py
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden                                             # noqa: E402  (placeholders, paths)
import gan_objective_fixture as FX                             # noqa: E402


def f16_emulation(model):
    """a copy of ``model`` whose convs see fp16-rounded weights and fp16-rounded inputs (fp32 arithmetic otherwise)"""
    m = copy.deepcopy(model)
    modules = m.modules() if isinstance(m, torch.nn.Module) else m.model.modules()
    for mod in modules:
        if isinstance(mod, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
            mod.weight.data = mod.weight.data.half().float()
            mod.register_forward_pre_hook(lambda _m, args: (args[0].half().float(),))
    return m


class Holder:
    """what the reference reaches through ``.model`` (netD.model.forward_multi, netF.model)"""

    def __init__(self, model):
        self.model = model

    def forward(self, *args, **kwargs):
        return self.model.forward(*args, **kwargs)

    __call__ = forward


class NoOptimizer:
    def zero_grad(self): pass
    def step(self): pass


class Networks:
    def __init__(self, networks):
        self.networks = networks


def main():
    make_golden._install_placeholders()
    sys.path.insert(0, make_golden.REF)
    threads = torch.get_num_threads()
    import mdir                                                     # noqa: F401
    torch.set_num_threads(threads)
    from mdir.components.model.network import hed as ref_hed, p2p_networks as ref_p2p
    from mdir.components.optim import criterion as ref_crit
    from mdir.learning import epoch_iteration as ref_epochs, network as ref_network
    from mdir.tools import gan_image_pool

    arrays = {}

    # ---- criterion cases
    for i in range(len(FX.CRITERION_SHAPES)):
        a, b = (t.double() for t in FX.criterion_maps(i))
        for label in ("l1", "mse"):
            arrays["c%d_%s" % (i, label)] = np.float64(ref_crit.CRITERIA[label]()(a, b))
        arrays["c%d_l1_sum" % i] = np.float64(ref_crit.CRITERIA["l1"](reduction="sum")(a, b))
    for i, (weights, normalize, heads) in enumerate(FX.MULTIHEAD_CASES):
        crit = ref_crit.initialize_criterion(FX.multihead_params("multihead_loss", weights, normalize, heads))
        maps = {key: [t.double() for t in FX.criterion_maps(v[1])] for key, v in heads.items()}
        out = crit({key: m[0] for key, m in maps.items()}, {key: m[1] for key, m in maps.items()})
        arrays["m%d_keys" % i] = np.array(list(out.partial.keys()))
        arrays["m%d_partial" % i] = np.array([float(v) for v in out.partial.values()], dtype=np.float64)
        arrays["m%d_total" % i] = np.float64(out.total)
        arrays["m%d_reduction" % i] = np.array(crit.reduction)
    for i, (weights, normalize, heads, at) in enumerate(FX.COMBINATION_CASES):
        crit = ref_crit.initialize_criterion(FX.multihead_params("combination_loss", weights, normalize, heads))
        a, b = (t.double() for t in FX.criterion_maps(at))
        out = crit(a, b)
        arrays["k%d_keys" % i] = np.array(list(out.partial.keys()))
        arrays["k%d_partial" % i] = np.array([float(v) for v in out.partial.values()], dtype=np.float64)
        arrays["k%d_total" % i] = np.float64(out.total)
    print("criterion cases: %d maps, %d multihead, %d combination" % (len(FX.CRITERION_SHAPES), len(FX.MULTIHEAD_CASES), len(FX.COMBINATION_CASES)))

    # ---- step cases
    def make_rcf(state):
        cuda = torch.Tensor.cuda
        torch.Tensor.cuda = lambda self, *a, **k: self               # RCF.__init__ builds its deconv kernels with .cuda() (make_rcf_golden.py)
        try:
            params = {"type": "SingleNetwork", "model": {"architecture": "rcf"}, "initialize": False, "runtime": {"wrappers": FX.RCFNGAN_WRAPPERS}}
            net = ref_network.initialize_network(params, "cpu").eval()
        finally:
            torch.Tensor.cuda = cuda
        net.model.load_state_dict(state)
        return net

    def held(label, nets):
        """the networks as the reference's step reaches them"""
        nets = dict(nets)
        for key in ("discriminator_X", "discriminator_Y") if label == "SupervisedCycleGanEpoch" else ("featdown",):
            if key in nets:
                nets[key] = Holder(nets[key])
        return nets

    def double(net):
        if isinstance(net, torch.nn.Module):
            return copy.deepcopy(net).double()
        net = copy.deepcopy(net)
        net.model.double()
        for key, value in list(vars(net.model).items()):             # RCF keeps its deconv kernels as plain tensor attributes (rcf.py:69-72)
            if torch.is_tensor(value):
                setattr(net.model, key, value.double())
        return net

    def run_step(label, nets, X, Y, recorded=None):
        epoch = ref_epochs.EPOCH_ITERATIONS[label].__new__(ref_epochs.EPOCH_ITERATIONS[label])
        epoch.criterion = ref_crit.initialize_criterion(FX.criterion_params(label))
        epoch.fake_X_pool, epoch.fake_Y_pool = gan_image_pool.GanImagePool(0), gan_image_pool.GanImagePool(0)
        nets = held(label, nets)
        if recorded is not None:
            inner = nets["featdown"].model

            def recording(feats, num_patches=64, patch_ids=None):
                out, ids = inner(feats, num_patches=num_patches, patch_ids=patch_ids)
                if patch_ids is None:
                    recorded.append(ids)
                return out, ids
            nets["featdown"] = Holder(recording)
        optimizers = {key: NoOptimizer() for key in nets}
        np.random.seed(FX.CUT_IDS_SEED)
        backward = torch.Tensor.backward
        if X.dtype == torch.float64:
            # the adversarial target tensor is fp32 (compound_losses.py:50): autograd refuses the mixed pair, the forward promotes it.  Nothing updates,
            # so the float64 run goes without the backward passes
            torch.Tensor.backward = lambda self, *a, **k: None
        try:
            losses, _ = epoch._optimization_step(Networks(nets), optimizers, "cpu", X, Y)
        finally:
            torch.Tensor.backward = backward
        for net in nets.values():
            model = getattr(net, "model", net)
            if isinstance(model, torch.nn.Module):
                model.zero_grad()
        return losses

    def maps_of(label, nets, X, Y):
        """every map a term of the scenario reads"""
        call = lambda net, x, **kw: net.forward(x, **kw)
        with torch.no_grad():
            if label == "SupervisedCycleGanEpoch":
                G_X, G_Y, D_X, D_Y = (nets[k] for k in ("generator_X", "generator_Y", "discriminator_X", "discriminator_Y"))
                fake_Y, fake_X = G_X(X), G_Y(Y)
                return {"pred_X_real": D_X(Y), "pred_X_fake": D_X(fake_Y), "pred_Y_real": D_Y(X), "pred_Y_fake": D_Y(fake_X), "rec_X": G_Y(fake_Y),
                        "rec_Y": G_X(fake_X)}
            G, D = nets["generator_X"], nets["discriminator_Y"]
            if label == "SupervisedCUTEpoch":
                fake = G(torch.cat((X, Y), dim=0))
                return {"pred_real": D(Y), "pred_fake": D(fake[:X.shape[0]]), "fake_Y": fake[:X.shape[0]], "idt_Y": fake[X.shape[0]:]}
            fake_Y = G(X)
            out = {"pred_real": D(Y), "pred_fake": D(fake_Y)}
            S = nets["detector"]
            out["fake_M"], out["real_M"] = call(S, fake_Y, no_sigmoid=True), call(S, X, no_sigmoid=True)
            if label == "SupervisedHEDNGANEpoch":
                out["target_M"] = call(nets["detector_frozen"], X, no_sigmoid=True)
            for key in ("fake_M", "real_M", "target_M"):
                if key in out:
                    out["sig_" + key] = torch.sigmoid(out[key])
            return out

    def nce_rows(label, nets, maps, X, Y, ids_nce, ids_idt):
        """per-row losses of the two patch-NCE terms with the stored ids: [nce layers], [idt layers]"""
        crit = ref_crit.initialize_criterion(FX.criterion_params(label))
        nce = crit.losses["nce"]
        G, F = nets["generator_X"], nets["featdown"]
        rows = []
        with torch.no_grad():
            for output, target, ids in ((X, maps["fake_Y"], ids_nce), (Y, maps["idt_Y"], ids_idt)):
                feat_q = G.forward(target, layers=nce.nce_layers, encode_only=True)
                feat_k = G.forward(output, layers=nce.nce_layers, encode_only=True)
                k_pool, _ = F(feat_k, num_patches=nce.num_patches, patch_ids=ids)
                q_pool, _ = F(feat_q, num_patches=nce.num_patches, patch_ids=ids)
                rows.append([c(q, k) for c, q, k in zip(nce.losses, q_pool, k_pool)])
        return rows

    T = lambda t: t.detach().cpu().numpy()
    for i, (name, label, norm, shape, detector) in enumerate(FX.STEP_CASES):
        p = name + "_"
        X, Y = FX.step_inputs(i)
        nets = FX.step_networks(i, ref_p2p, ref_hed.HedInterpolation, make_rcf)
        recorded = [] if label == "SupervisedCUTEpoch" else None
        f32 = run_step(label, nets, X, Y, recorded)
        f64 = run_step(label, {k: double(v) for k, v in nets.items()}, X.double(), Y.double(), None if recorded is None else [])
        assert list(f32) == list(f64)
        arrays[p + "keys"] = np.array(list(f32))
        arrays[p + "f32"] = np.array([f32[k] for k in f32], dtype=np.float64)
        arrays[p + "f64"] = np.array([f64[k] for k in f64], dtype=np.float64)
        arrays[p + "shape"] = np.array(shape, dtype=np.int64)
        maps = maps_of(label, nets, X, Y)
        emu_nets = {k: f16_emulation(v) for k, v in nets.items()}
        emu = maps_of(label, emu_nets, X, Y)
        for key in maps:
            if key not in ("fake_Y", "idt_Y"):
                arrays[p + "emu_" + key] = np.float64((maps[key] - emu[key]).abs().max())
        if label == "SupervisedCycleGanEpoch":
            adv = ref_crit.initialize_criterion(FX.criterion_params(label)).loss_D_X
            for s in ("X", "Y"):
                arrays[p + "aux_D_%s_real" % s] = np.float64(adv(maps["pred_%s_real" % s], True, "cpu").total)
                arrays[p + "aux_D_%s_fake" % s] = np.float64(adv(maps["pred_%s_fake" % s], False, "cpu").total)
        if label == "SupervisedCUTEpoch":
            ids_nce, ids_idt = recorded
            for tag, ids in (("nce", ids_nce), ("idt", ids_idt)):
                for l, t in enumerate(ids):
                    arrays[p + "ids_%s%d" % (tag, l)] = T(t).astype(np.int32)
            rows = nce_rows(label, nets, maps, X, Y, ids_nce, ids_idt)
            rows_emu = nce_rows(label, emu_nets, emu, X, Y, ids_nce, ids_idt)
            for tag, r, re in zip(("nce", "idt"), rows, rows_emu):
                arrays[p + tag + "_f16_emulated_row_err"] = np.array([float((a - b).abs().max()) for a, b in zip(r, re)])
                arrays[p + tag + "_layer_means"] = np.array([float(a.mean()) for a in r], dtype=np.float64)
        gates, L = FX.step_gates(i, arrays)
        print("step case %s %s %s %s:" % (name, label, norm, shape))
        for key in f32:
            print("    %-22s f32 %.6f  f64 %.6f  |d| %.1e  gate %.3e" % (key, f32[key], f64[key], abs(f32[key] - f64[key]), gates[key]))
        print("    emu: " + ", ".join("%s %.2e" % (k[len(p) + 4:], float(v)) for k, v in arrays.items() if k.startswith(p + "emu_")))
        for a, b in () if name in FX.PLAIN_GAIN_CASES else FX.EXCHANGEABLE[label]:
            apart, room = abs(L[a] - L[b]), gates[a] + gates[b]
            print("    |%s - %s| = %.3e against gates %.3e" % (a, b, apart, room))
            assert apart > room, (name, a, b, apart, room)
    path = os.path.join(HERE, "gan_objective.npz")
    np.savez_compressed(path, **arrays)
    print("wrote gan_objective.npz %.1f KiB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
