"""The pix2pix U-Net generator mirror and the ``reflectpad_divisible`` wrapper on the host (no GPU): registry, module tree and state-dict keys, the fp32 map in
front of the Tanh against the fixture the reference wrote (tests/golden/make_unet_golden.py), the in-place LeakyReLU on the skip tensor, Dropout
in eval mode, the rejected sizes and precisions, the wrapper's padding, padded tensors and crops bit for bit."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from gandtr_amd.tools import synth

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet.npz"))
N_CASES = int(GOLD["n_cases"])


def case(i):
    """(mirror in eval mode with the fixture's seeded weights, seeded input, fixture prefix)"""
    from gandtr_amd.components.model.network import p2p_networks
    p = "c%d_" % i
    num_downs, ngf, dropout, wseed, xseed = (int(v) for v in GOLD[p + "cfg"])
    norm = str(GOLD[p + "norm"])
    model = p2p_networks.UnetGenerator(3, 3, num_downs, ngf=ngf, norm_layer=norm, use_dropout=bool(dropout)).eval()
    model.load_state_dict(synth.unet_state(wseed, norm, ngf=ngf, num_downs=num_downs, gain=float(GOLD["gain"])), strict=True)
    x = synth.synth_input(xseed, tuple(int(v) for v in GOLD[p + "shape"]), 1.0)
    return model, x, p


def pre_tanh(model, x):
    seen = []
    h = model.model.model[-2].register_forward_hook(lambda _m, _i, o: seen.append(o.clone()))
    with torch.no_grad():
        y = model(x.clone())
    h.remove()
    return seen[0], y


def test_registry_label_and_constructor_defaults():
    import inspect
    from gandtr_amd.components.model import network as registry
    from gandtr_amd.components.model.network import p2p_networks
    assert registry.MODEL_LABELS["official_p2p_unet_generator"] is p2p_networks.UnetGenerator
    sig = inspect.signature(p2p_networks.UnetGenerator.__init__)
    assert list(sig.parameters)[1:] == ["input_nc", "output_nc", "num_downs", "ngf", "norm_layer", "use_dropout", "track_running_stats"]
    assert [sig.parameters[k].default for k in ("ngf", "norm_layer", "use_dropout", "track_running_stats")] == [64, "batch", False, True]
    model = registry.initialize_model({"architecture": "official_p2p_unet_generator", "input_nc": 3, "output_nc": 2, "num_downs": 5, "ngf": 8})
    assert model.meta == {"in_channels": 3, "out_channels": 2}
    assert isinstance(model.model, p2p_networks.UnetSkipConnectionBlock) and model.hip_default_precision == "f16"
    with torch.no_grad():
        assert tuple(model.eval()(synth.synth_input(1, (1, 3, 32, 64), 1.0)).shape) == (1, 2, 32, 64)


@pytest.mark.parametrize("i", range(N_CASES))
def test_state_dict_keys_and_shapes_are_the_references(i):
    model, _, p = case(i)
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in GOLD[p + "keys"]]
    shapes = [list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()]
    assert shapes == GOLD[p + "shapes"].tolist()
    from gandtr_amd import engine
    num_downs, ngf = int(GOLD[p + "cfg"][0]), int(GOLD[p + "cfg"][1])
    assert engine.unet_layout(sd) == (str(GOLD[p + "norm"]), ngf, num_downs, 3, 3)


@pytest.mark.parametrize("i", range(N_CASES))
def test_cpu_forward_reproduces_the_reference(i):
    """the same torch ops on the same weights: within 1e-5 of the range (Dropout case included: eval mode)"""
    model, x, p = case(i)
    pre, y = pre_tanh(model, x)
    ref = torch.from_numpy(GOLD[p + "pre"])
    assert pre.shape == ref.shape == x.shape
    rel = float((pre - ref).abs().max() / ref.abs().max())
    assert rel <= 1e-5, rel
    assert float(ref.abs().max()) == pytest.approx(float(GOLD[p + "pre_max"])) and 0.5 <= float(GOLD[p + "pre_max"]) <= 20.0
    assert float((y[:, :, ::4, ::4] - torch.from_numpy(GOLD[p + "tanh_sub"])).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_dropout_case_has_dropout_and_is_identity_in_eval():
    model, x, p = case(5)
    assert int(GOLD[p + "cfg"][2]) == 1 and sum(isinstance(m, nn.Dropout) for m in model.modules()) == 1       # num_downs 6: one ngf * 8 intermediate block
    a, _ = pre_tanh(model, x)
    b, _ = pre_tanh(model, x)
    assert torch.equal(a, b)


def test_inplace_leaky_relu_on_the_skip_tensor_is_pinned():
    """The LeakyReLU at the head of a block is IN PLACE, as in the reference: it rewrites the block's input before torch.cat reads it, so a non-outermost
    block returns cat([leaky(x), up]) -- checked here on the block itself, where it shows.  At the net's output it cannot show: the parent's ReLU follows
    the concatenation and relu(leaky(x)) = relu(x) bit for bit, so a variant of the mirror whose activations are not in place reproduces the fixture
    exactly (asserted too).  That identity is what lets the device graph store ONE down tensor per level (engine.build_unet_generator)."""
    import copy
    model, x, p = case(0)
    block = model.model.model[1]                               # the first non-outermost block
    with torch.no_grad():
        d0 = model.model.model[0](x)                           # the outermost down conv's output: negative values present
        assert float(d0.min()) < 0
        want_skip = torch.nn.functional.leaky_relu(d0, 0.2)
        fed = d0.clone()
        out = block(fed)
    c = d0.shape[1]
    assert torch.equal(out[:, :c], want_skip) and not torch.equal(out[:, :c], d0)
    assert torch.equal(fed, want_skip)                         # the caller's tensor itself was rewritten
    variant = copy.deepcopy(model)
    for m in variant.modules():
        if isinstance(m, (nn.LeakyReLU, nn.ReLU)):
            m.inplace = False
    with torch.no_grad():
        fed = d0.clone()
        out_v = variant.model.model[1](fed)
    assert torch.equal(out_v[:, :c], d0) and torch.equal(fed, d0)          # not in place: the raw tensor is concatenated
    ref = torch.from_numpy(GOLD[p + "pre"])
    pre_m, _ = pre_tanh(model, x)
    pre_v, _ = pre_tanh(variant, x)
    assert float((pre_m - ref).abs().max() / ref.abs().max()) <= 1e-5
    assert torch.equal(pre_m, pre_v)                           # ... and the parent's ReLU hides it


def test_non_divisible_size_raises_on_the_reference_path():
    model, _, _ = case(1)                        # num_downs 5
    with torch.no_grad(), pytest.raises(RuntimeError):
        model(synth.synth_input(1, (1, 3, 48, 40), 1.0))
    with torch.no_grad():
        assert tuple(model(synth.synth_input(1, (1, 3, 32, 32), 1.0)).shape) == (1, 3, 32, 32)


def test_instance_norm_smallest_map_is_two_by_two():
    model, _, _ = case(0)                        # instance, num_downs 5
    with torch.no_grad():
        assert bool(torch.isfinite(model(synth.synth_input(1, (1, 3, 32, 32), 1.0))).all())


def test_generator_modes_are_refused_without_a_device(monkeypatch):
    from gandtr_amd import engine
    monkeypatch.delenv("GANDTR_HIP_PRECISION", raising=False)
    model, _, _ = case(1)
    sd = {k: v for k, v in model.state_dict().items()}
    for prec in ("f16c", "f16ch"):
        with pytest.raises(NotImplementedError):
            engine.build_unet_generator(sd, "cuda", precision=prec)
        model.hip_precision = prec
        with pytest.raises(NotImplementedError):
            model._hip_modes()
    model.hip_precision = None
    assert model._hip_modes() == "f16"


def test_c_abi_adder_validates_without_a_device():
    import ctypes
    from gandtr_amd import _hip
    lib = _hip.load()
    h, out = ctypes.c_void_p(), ctypes.c_int()
    _hip.check(lib.gdt_net_create(ctypes.byref(h)))
    _hip.check(lib.gdt_net_input(h, 3, None, None, None, ctypes.byref(out)))
    w = np.zeros((8, 8, 4, 4), np.float32)
    wts = _hip.ConvWeights(w.ctypes.data)

    def t4(in_b, relu, act, res):
        d = _hip.ConvDesc(3, 8, 4, 4, 2, 1, 0, 1, relu, 0, act, 1e-5)          # cin: the channels of the input (the weight's first three rows are read)
        return lib.gdt_net_conv(h, out.value, in_b, ctypes.byref(d), ctypes.byref(wts), -1, ctypes.byref(res))
    with pytest.raises(ValueError):               # unknown second input
        _hip.check(t4(7, 0, 0, out))
    with pytest.raises(ValueError):               # an internal output takes no tanh
        _hip.check(t4(-1, 0, 1, out))
    t = ctypes.c_int()
    _hip.check(t4(-1, 1, 0, t))
    names = _hip.plan_count_names()
    counts = (ctypes.c_int * len(names))()
    _hip.check(lib.gdt_net_plan_summary(h, 1, 8, 8, 0, counts, len(names)))
    assert counts[names.index("conv_launches")] == 1 and counts[names.index("conv4x4t_launches")] == 0     # 8 channels: the generic route
    lib.gdt_net_destroy(h)


# ------------------------------------------------------------------------------------------------ reflectpad_divisible
def wrap_inputs():
    return [synth.synth_input(80 + k, s, 1.0) for k, s in enumerate(((1, 3, 50, 70), (1, 2, 20, 33)))]


def test_reflectpad_divisible_label_and_mini_dsl():
    from gandtr_amd.components.data import wrapper
    assert wrapper.WRAPPERS_LABELS["reflectpad_divisible"] is wrapper.ReflectPadMakeDivisible
    comp = wrapper.initialize_wrappers("reflectpad_divisible:32", "cpu")
    assert len(comp.wrappers) == 1 and isinstance(comp.wrappers[0], wrapper.ReflectPadMakeDivisible) and comp.wrappers[0].divisible_by == 32
    comp = wrapper.initialize_wrappers({"0_reflectpad_divisible": {"divisible_by": 16}}, "cpu")
    assert comp.wrappers[0].divisible_by == 16


def test_reflectpad_divisible_matches_the_reference_bit_for_bit():
    from gandtr_amd.components.data import wrapper
    w = wrapper.ReflectPadMakeDivisible("32", "cpu")
    xs = wrap_inputs()
    padded, padding = w.preprocess(xs[0], None)
    assert tuple(padding) == tuple(int(v) for v in GOLD["wrap_padding"]) == (13, 13, 7, 7)
    assert torch.equal(padded, torch.from_numpy(GOLD["wrap_padded"])) and tuple(padded.shape) == (1, 3, 64, 96)
    assert torch.equal(w.postprocess(padded, None, padding), xs[0])
    assert torch.equal(padded[0, :, 0, 0], xs[0][0, :, 0, 0])                     # despite the name, the border is REPLICATED
    lp, lpad = w.preprocess(list(xs), None)
    assert isinstance(lp, list) and isinstance(lpad, list)
    assert [tuple(p) for p in lpad] == [tuple(int(v) for v in row) for row in GOLD["wrap_list_padding"]] == [(13, 13, 7, 7), (15, 16, 6, 6)]
    assert torch.equal(lp[0], padded) and torch.equal(lp[1], torch.from_numpy(GOLD["wrap_list_padded1"]))
    crops = w.postprocess(lp, None, lpad)
    assert torch.equal(crops[0], xs[0]) and torch.equal(crops[1], torch.from_numpy(GOLD["wrap_list_crop1"])) and torch.equal(crops[1], xs[1])
    # a size that is divisible already: no padding, and the crop with "-0 or None" keeps everything
    y, pad0 = w.preprocess(torch.zeros(1, 1, 32, 64), None)
    assert pad0 == (0, 0, 0, 0) and tuple(w.postprocess(y, None, pad0).shape) == (1, 1, 32, 64)


def test_wrapped_net_on_the_cpu_matches_the_reference():
    from gandtr_amd.components.data import wrapper
    model, _, _ = case(0)
    comp = wrapper.initialize_wrappers("reflectpad_divisible:32", "cpu")
    with torch.no_grad():
        y = comp(wrap_inputs()[0], model, outputmodel=model)
    ref = torch.from_numpy(GOLD["wrap_net_out"])
    assert y.shape == ref.shape == (1, 3, 50, 70)
    assert float((y - ref).abs().max()) <= 1e-5 * float(GOLD["wrap_net_pre_max"])
