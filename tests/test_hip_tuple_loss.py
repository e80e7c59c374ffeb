"""The tuple loss on the device (gdt_tuple_loss, gandtr_amd/csrc/tuple_loss.hip) and the loss validation of the fine-tuning scenario end to end.

Kernel: against the reference's own values (tests/golden/tuple_loss.npz) and against the float64 evaluation of the same formulas on the same
fp32 inputs, with the bound derived in tests/test_tuple_loss_host.py (relative d * 2^-24 on a squared distance, carried through the formula;
``test_reference_fp32_sits_inside_the_bound`` there shows that the reference's fp32 results keep it too).  Sizes: d = 8 / 100 / 2048 on 16-byte
loads (100: the wave's tail lanes idle, row stride no multiple of 256 bytes), d = 7 on scalar loads; S = 2 / 3 / 7 (one to six waves per
workgroup); 1 / 3 / 257 tuples."""
import copy

import numpy as np
import pytest
import torch

from gandtr_amd import mining
from gandtr_amd.components.optim import criterion as C
from gandtr_amd.tools import synth, tensors
from test_tuple_loss_host import (FINETUNE_CRITERION, FINETUNE_DATA_VAL, FINETUNE_EMBED_DATA, FINETUNE_VALIDATION, FINETUNE_WRAPPERS, GOLDEN, bounds,
                                  criterion_of, float64_losses, load_cases)

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("d", [8, 100, 2048, 7])
def test_kernel_against_the_fixture_and_float64(cuda_device, d, kind):
    cases = [c for c in load_cases() if c["d"] == d]
    assert len(cases) == (10 if d == 100 else 9)                          # S x T, and the crafted tuples on the d = 100 pool
    worst = 0.0
    for c in cases:
        margin, ref_tuple, ref_batch = c[kind]
        crit = criterion_of(kind, margin)
        want = float64_losses(c["pool"], c["table"], kind, margin)
        tol = bounds(want, d, kind, margin)
        got = crit.tuple_losses(torch.from_numpy(c["pool"]).to(cuda_device), c["table"], with_pairs=True)
        loss, pair, total = got.loss.cpu().double().numpy(), got.pair_dist.cpu().double().numpy(), float(got.total)
        err = np.abs(loss - want["loss"])
        worst = max(worst, float((err / np.maximum(tol["loss"], 1e-300)).max()))
        assert (np.abs(pair - want["pair"]) <= tol["pair"]).all(), c["name"]
        assert (err <= tol["loss"]).all(), c["name"]
        assert abs(total - want["total"]) <= tol["total"], c["name"]
        # the reference's fp32 values lie within the same bound of float64: within twice the bound of the kernel's
        assert (np.abs(loss - ref_tuple) <= 2 * tol["loss"]).all(), c["name"]
        assert abs(total - ref_batch) <= 2 * tol["total"] + abs(want["total"]) * 2.0 ** -23, c["name"]
        # the total is the float64 sum of the returned tuple losses, to float64 rounding (another order of the same additions)
        assert abs(total - float(loss.sum())) <= len(loss) * 2.0 ** -52 * float(np.abs(loss).sum()), c["name"]
    print("d=%d kind=%d: the kernel uses at most %.3f of the bound" % (d, kind, worst))


def test_crafted_tuples(cuda_device):
    c = [c for c in load_cases() if c["name"] == "crafted"][0]
    got = C.ContrastiveLoss(0.75).tuple_losses(torch.from_numpy(c["pool"]).to(cuda_device), c["table"], with_pairs=True)
    pair, loss = got.pair_dist.cpu().numpy(), got.loss.cpu().numpy()
    eps = np.float32(1e-6)
    assert pair[0, 0] == pytest.approx(10 * float(eps), rel=100 * 2.0 ** -24) and pair[0, 0] > 0     # sqrt(100) eps: eps inside the difference
    assert (pair[1, 1:] > 0.75).all() and loss[1] == np.float32(0.5) * (pair[1, 0] * pair[1, 0])      # zero hinge: exactly the positive term
    assert c["table"][2, 0] == c["table"][3, 0] and loss[2] != loss[3]


def test_two_calls_and_a_permuted_table_give_the_same_bits(cuda_device):
    c = [c for c in load_cases() if c["name"] == "d100_s7_t257"][0]
    pool = torch.from_numpy(c["pool"]).to(cuda_device)
    perm = torch.randperm(257, generator=torch.Generator().manual_seed(0))
    for kind, margin in ((0, 0.75), (1, 0.1)):
        crit = criterion_of(kind, margin)
        a = crit.tuple_losses(pool, c["table"], with_pairs=True)
        b = crit.tuple_losses(pool, c["table"], with_pairs=True)
        for x, y in zip(a, b):
            assert torch.equal(_bits(x), _bits(y))
        p = crit.tuple_losses(pool, c["table"][perm.numpy()], with_pairs=True)
        assert torch.equal(_bits(p.loss), _bits(a.loss)[perm]) and torch.equal(_bits(p.pair_dist), _bits(a.pair_dist)[perm])
        # a tuple's loss does not depend on the table around it, a table on the device is taken as it is, pair_dist is optional
        one = crit.tuple_losses(pool, torch.from_numpy(c["table"][100:101]).to(cuda_device))
        assert one.pair_dist is None and torch.equal(_bits(one.loss), _bits(a.loss)[100:101])


@pytest.mark.parametrize("d", [100, 7])
def test_label_form_gives_the_bits_of_the_index_form(cuda_device, d):
    c = [c for c in load_cases() if c["name"] == "d%d_s7_t3" % d][0]
    pool = torch.from_numpy(c["pool"]).to(cuda_device)
    x = pool[:, torch.from_numpy(c["table"].reshape(-1)).long().to(cuda_device)]           # D x 21: the tuples side by side, as the reference gets them
    label = torch.from_numpy(c["label"])
    for kind, margin in ((0, 0.75), (1, 0.1)):
        crit = criterion_of(kind, margin)
        index = crit.tuple_losses(pool, c["table"])
        got = crit(x, label)
        assert got.is_cuda and got.dim() == 0 and got.dtype == torch.float32
        assert torch.equal(_bits(got), _bits(index.total.float()))
        assert torch.equal(_bits(crit(x, [label[i:i + 7].to(cuda_device) for i in range(0, 21, 7)])), _bits(got))
        assert torch.equal(_bits(crit.tuple_losses(x, torch.arange(21).reshape(3, 7)).loss), _bits(index.loss))


def test_bad_tables_raise_before_any_launch(cuda_device):
    pool = torch.from_numpy(load_cases()[0]["pool"]).to(cuda_device)
    crit = C.ContrastiveLoss(0.75)
    for bad in ([[0, 300]], [[-1, 2]], [[0]], [], [[0.5, 1.0]]):
        with pytest.raises(ValueError):
            crit.tuple_losses(pool, bad)
    with pytest.raises(ValueError):
        crit(pool[:, :6], torch.tensor([-1., 1, 0, -1, 0, 1]))


# ---- end to end, tiny: 12 images in 4 clusters, 4 tuples of (anchor, positive, 2 negatives), GeM-VGG16 with seeded weights

EMBED = {"type": "SingleNetwork",
         "model": {"architecture": "cirnet", "cir_architecture": "vgg16", "local_whitening": False, "pooling": "gem", "pretrained": False,
                   "regional": False, "whitening": False},
         "initialize": False, "runtime": {"wrappers": "cirfaketuplebatch", "data": dict(FINETUNE_EMBED_DATA)}}
AUGMENT = {"type": "SingleNetwork",
           "model": {"architecture": "official_resnet_generator", "input_nc": 3, "output_nc": 3, "n_blocks": 9, "norm_layer": "instance",
                     "no_antialias": True, "no_antialias_up": True},
           "initialize": False,
           "runtime": {"frozen": True, "wrappers": FINETUNE_WRAPPERS,
                       "data": {"transforms": "pil2np | totensor | normalize", "mean_std": [[0.5] * 3, [0.5] * 3]}}}

# |loss(batched validation) - loss(the reference's loop shape: one tuple per forward, torch formula)| over the four tuples, measured once on an
# MI355X at this geometry: batched and single launches choose different kernel forms, so this is a tolerance and not bits
MEASURED_GAP = {"embed": 2.03e-5, "chain": 3.32e-5}


def _dataset():
    """12 images (64 x 64 and 64 x 80 tensors) in 4 clusters; the anchors are named so that the md5 rule passes two of the four"""
    g = np.load(GOLDEN)
    names, decisions = [str(n) for n in g["pass_names"]], g["pass_decisions"].tolist()
    yes, no = [n for n, d in zip(names, decisions) if d], [n for n, d in zip(names, decisions) if not d]
    cids = [None] * 12
    for k, q in enumerate((0, 3, 6, 9)):
        cids[q] = yes[k // 2] if k % 2 == 0 else no[k // 2]
    rest = iter(yes[2:] + no[2:])
    cids = [c if c is not None else next(rest) for c in cids]
    images = [synth.synth_input(20 + i, (3, 64, 64 if i % 2 else 80), 1.0) for i in range(12)]
    db = {"qidxs": [0, 3, 6, 9], "pidxs": [1, 4, 7, 10], "cluster": [i // 3 for i in range(12)], "cids": cids}
    passing = {q for q in db["qidxs"] if decisions[names.index(cids[q])]}
    assert len(passing) == 2
    return db, images, passing


def _network(kind, device):
    from gandtr_amd.learning import network as N
    if kind == "embed":
        net = N.initialize_network(copy.deepcopy(EMBED), device).eval()
        net.model.load_state_dict(synth.vgg16_state(0))
        return net
    net = N.initialize_network({"type": "CirSequentialNetwork", "sequence": "augment,embed", "augment": copy.deepcopy(AUGMENT),
                                "embed": copy.deepcopy(EMBED)}, device).eval()
    net.networks["augment"].model.load_state_dict(synth.generator_state(0, "instance", gain=0.02))
    net.networks["embed"].model.load_state_dict(synth.vgg16_state(0))
    return net


def _gate_bound(pair, margin=0.75, d=512, gate=1e-3):
    """what the project's descriptor gate (|delta|_inf <= 1e-3 per descriptor) allows a tuple's contrastive loss to move: a pair distance moves
    by at most |delta_a - delta_b|_2 <= 2 sqrt(d) gate, a term 0.5 x^2 by x dx + 0.5 dx^2"""
    dx = 2 * np.sqrt(d) * gate
    x = np.concatenate([pair[:, :1], np.maximum(margin - pair[:, 1:], 0)], axis=1)
    return (x * dx + 0.5 * dx * dx).sum(1)


@pytest.mark.parametrize("kind", ["embed", "chain"])
def test_validation_end_to_end(cuda_device, kind):
    """``SingleValidation.validate`` on finetune.yml's validation section.  Against the reference's loop shape (every tuple alone through
    ``network.forward``, torch formula) the largest gap of a tuple's loss measured on an MI355X is 2.03e-5 (embedder alone) and 3.32e-5 (augment,
    embed chain), MEASURED_GAP; the assertion uses twice that value, which lies far below what the descriptor gate would allow
    (``_gate_bound``: about 0.07 per tuple here)."""
    from gandtr_amd.learning.validation import initialize_validation
    from gandtr_amd.stages.validate import extract_vectors
    db, images, passing = _dataset()
    net = _network(kind, cuda_device)
    crit = C.initialize_criterion(dict(FINETUNE_CRITERION))
    data_val = copy.deepcopy(FINETUNE_DATA_VAL)
    data_val["dataset"].update(query_size=4, neg_num=2, image_size=80)
    val = initialize_validation(copy.deepcopy(FINETUNE_VALIDATION), data={"db": db, "images": images}, params_data={"val": data_val},
                                default_criterion=crit, network=net)
    rows = []
    torch.manual_seed(3)
    acc = val.validate(net, cuda_device, lambda *row: rows.append(row))
    assert isinstance(acc, list) and len(acc) == 4 and all(isinstance(x, float) and np.isfinite(x) for x in acc)
    assert rows[0][2] == "data_mining" and len(rows[0][3]["average_negative_distance"]) == 8
    data = val.data_loader
    assert sorted(data.qidxs) == db["qidxs"]
    for q, negs in zip(data.qidxs, data.nidxs):
        cl = [db["cluster"][n] for n in negs]
        assert len(negs) == 2 and len(set(cl)) == 2 and db["cluster"][q] not in cl
    # bit for bit: tuple_losses on what extract_vectors returns for the same distinct (image, label) entries
    entries, table = mining.epoch_tuple_table(data.qidxs, data.pidxs, data.nidxs, data.tuple_labels)
    meta = [{"image_label": label, "name": db["cids"][i]} for i, label in entries]
    vecs = extract_vectors(net, [images[i] for i, _ in entries], cuda_device, metadata=meta)
    again = crit.tuple_losses(vecs, table, with_pairs=True)
    assert again.loss.cpu().tolist() == acc
    if kind == "chain":
        # which images went through the generator: exactly the anchors the md5 rule selects.  A skipped image is still post-processed by the wrappers
        # listed before the pass-through (the reference runs postprocess in reverse order: CLAHE, then the mean / std change), so the comparison is with
        # the embedder alone on the images put through those two by hand
        chain = net.networks["augment"].wrappers["eval"].wrappers
        by_hand = [chain[0].postprocess(chain[1].postprocess(images[i][None].to(cuda_device), None, None), None, None) for i, _ in entries]
        plain = extract_vectors(net.networks["embed"], by_hand, cuda_device)
        delta = (vecs - plain).abs().max(dim=0).values.cpu().tolist()
        print("chain vs embedder alone, max |delta| per entry:", ["%s:%s %.2e" % (i, l, x) for (i, l), x in zip(entries, delta)])
        for (i, label), x in zip(entries, delta):
            if label == "anc" and i in passing:
                assert x > 1e-2, (i, label, x)
            else:
                assert x <= 1e-3, (i, label, x)
    # the reference's loop shape: each tuple alone through network.forward (batch-1 forwards), the torch formula on the host
    loop = []
    with torch.no_grad():
        for t in range(4):
            tuple_images = [tensors.as_metadata_tensor(images[i][None].clone(), {"image_label": [label], "name": [db["cids"][i]]})
                            for i, label in (entries[k] for k in table[t].tolist())]
            x = net.forward(tuple_images)
            assert x.shape == (512, 4)
            loop.append(float(crit(x.cpu(), torch.tensor([-1., 1, 0, 0]))))
    gap = max(abs(a - b) for a, b in zip(acc, loop))
    gate = _gate_bound(again.pair_dist.cpu().double().numpy())
    print("%s: losses %s, loop %s, gap %.3e, gate bound %s" % (kind, acc, loop, gap, gate.tolist()))
    assert all(abs(a - b) <= g for a, b, g in zip(acc, loop, gate))
    if MEASURED_GAP[kind] is not None:
        assert 2 * MEASURED_GAP[kind] < gate.min()                        # the assertion below is the tighter of the two bounds
        assert gap <= 2 * MEASURED_GAP[kind]
