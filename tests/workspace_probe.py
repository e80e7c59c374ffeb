"""Shared by tests/test_workspace_layout_host.py and tests/test_hip_workspace.py: the knob environment, the nets beyond test_plan_routes_host.NETS whose plans take
the routes those families never take (Bottleneck launches, 3x3 + expand with the chained reduce, the K-concatenated shortcut, fused BasicBlocks, the heads with a
scratch of their own, the blur op with a folded norm), and ``probe`` -- one forward on a caller-made workspace of known content between two guard bands.

What the graph workspace holds (Planner::layout, csrc/net_plan.hip; the executor's reads of Step::aux_off, csrc/net_exec.hip): activation tensors in fp16 or
fp32, fp32 statistics slabs and (mean, rstd) rows, fp32 scratch of the row-split head, the GeM / pool / median / local heads and the HED / RCF score maps.  No
index, counter or pointer lives there, so a byte pattern can change a value a launch reads but never an address."""
import contextlib
import os

import pytest
import torch

from gandtr_amd import engine
from gandtr_amd.engine import HipNet
from gandtr_amd.tools import synth

NO_REUSE = "GDT_PLAN_NO_REUSE"
# byte patterns: zeros; NaN as fp16 and as fp32; 0x7B7B = 61280 as fp16, 0x7B7B7B7B ~ 1.3e36 as fp32 -- large and finite, so it survives the fmax / ReLU that swallow a NaN
FILLS = (0x00, 0xFF, 0x7B)
GUARD = 64 << 10          # bytes of each guard band: a multiple of the planner's 256-byte alignment, so that the slice between them is aligned as torch's allocation is
DEV = "cuda:0"            # only recorded until finalize()


@contextlib.contextmanager
def knobs(settings):
    """no GDT_* and no GANDTR_HIP_* variable but ``settings`` for the duration"""
    saved = {k: v for k, v in os.environ.items() if k.startswith(("GDT_", "GANDTR_HIP_"))}
    for k in saved:
        del os.environ[k]
    os.environ.update(settings)
    try:
        yield
    finally:
        for k in settings:
            os.environ.pop(k, None)
        os.environ.update(saved)


def _g(name, shape, std):
    return synth._normal(0, name, shape, std)


def _finish(net, finalize):
    return net.finalize() if finalize else net


def block_net(C, mid, nblocks, dev=DEV, finalize=False):
    """the identity Bottleneck chain of tests/test_hip_bneck.py::_block_net: 1x1 stem to C channels, then ``nblocks`` blocks C -> mid -> mid -> C, every block tapped"""
    net = HipNet(dev, "f16")
    x = net.conv(net.input(3), _g("w0", (C, 3, 1, 1), 0.5), _g("b0", (C,), 0.3), relu=True)
    net.output_nchw(x)
    for b in range(nblocks):
        r = net.conv(x, _g("wr%d" % b, (mid, C, 1, 1), C ** -0.5), _g("br%d" % b, (mid,), 0.2), relu=True)
        t3 = net.conv(r, _g("w3%d" % b, (mid, mid, 3, 3), (9 * mid) ** -0.5), _g("b3%d" % b, (mid,), 0.2), pad=1, relu=True)
        x = net.conv(t3, _g("we%d" % b, (C, mid, 1, 1), mid ** -0.5), _g("be%d" % b, (C,), 0.2), relu=True, residual=x)
        net.output_nchw(x)
    return _finish(net, finalize)


def projection_net(cin, mid, C, stride, dev=DEV, finalize=False):
    """the first block of a ResNet stage as in tests/test_hip_bneck.py: 1x1 projection shortcut (emitted first, as engine.py does), reduce, 3x3 (carrying the
    stride), expand + shortcut"""
    net = HipNet(dev, "f16")
    x = net.conv(net.input(3), _g("w0", (cin, 3, 1, 1), 0.5), _g("b0", (cin,), 0.3), relu=True)
    net.output_nchw(x)
    sc = net.conv(x, _g("wd", (C, cin, 1, 1), cin ** -0.5), _g("bd", (C,), 0.2), stride=stride)
    r = net.conv(x, _g("wr", (mid, cin, 1, 1), cin ** -0.5), _g("br", (mid,), 0.2), relu=True)
    t3 = net.conv(r, _g("w3", (mid, mid, 3, 3), (9 * mid) ** -0.5), _g("b3", (mid,), 0.2), stride=stride, pad=1, relu=True)
    y = net.conv(t3, _g("we", (C, mid, 1, 1), mid ** -0.5), _g("be", (C,), 0.2), relu=True, residual=sc)
    net.output_nchw(y)
    return _finish(net, finalize)


def _head_state():
    """ResNet-18 trunk (512-channel map) with every layer a head can ask for: the regional whitening, the final whitening, per-channel exponents unused"""
    sd = synth.resnet_basic_state(0)
    for key in ("pool.whiten", "whiten"):
        sd[key + ".weight"], sd[key + ".bias"] = _g(key + ".w", (512, 512), 512 ** -0.5), _g(key + ".b", (512,), 0.1)
    sd["pool.rpool.p"] = sd["pool.p"]
    return sd


def _embedder(state, **kw):
    return lambda dev=DEV, finalize=False: engine.build_embedder(state(), dev, finalize=finalize, **kw)


def _generator(precision, **state_kw):
    return lambda dev=DEV, finalize=False: engine.build_generator(synth.generator_state(0, **state_kw), dev, precision=precision, finalize=finalize)


def _blocks(C, mid, nblocks):
    return lambda dev=DEV, finalize=False: block_net(C, mid, nblocks, dev, finalize)


def _projection(cin, mid, C, stride):
    return lambda dev=DEV, finalize=False: projection_net(cin, mid, C, stride, dev, finalize)


# one builder object per net: the device tests build each once and share it among its cases
GEN_C, GEN_X3 = _generator("f16c"), _generator("f16x3")
R101, VGG, R18 = _embedder(lambda: synth.resnet101_state(0)), _embedder(lambda: synth.vgg16_state(0)), _embedder(lambda: synth.resnet_basic_state(0))
B256, B1024, PROJ, PROJ_S2 = _blocks(256, 64, 2), _blocks(1024, 256, 3), _projection(64, 64, 256, 1), _projection(256, 128, 512, 2)
BASIC = {"GDT_CONV_BASIC": "2"}
X3_FORMS = {"GDT_CONV_HALO_X3": "2", "GDT_CONV_HALO_X3_FORMS": "2"}
AA = dict(ngf=64, n_blocks=2, no_antialias=False, no_antialias_up=False)       # the full-width anti-aliased generator of tests/test_hip_antialias_generator.py

# label -> (builder(dev, finalize), (n, h, w), knob settings besides GDT_PLAN_NO_REUSE, counters the plan must show: name -> least value; "basic" / "blur_folded"
# are basic_blocks_fused() and blur_summary()["folded"])
EXTRA = {
    "generator/f16c@4x128": (GEN_C, (4, 128, 128), {}, {"norms_folded": 23, "transposed_fused": 2, "stride2_shift": 2}),
    "generator/f16x3@2x64": (GEN_X3, (2, 64, 64), {}, {}),
    "generator/f16x3@2x64/forms": (GEN_X3, (2, 64, 64), X3_FORMS, {"norms_folded": 1, "stride2_shift": 2}),
    "generator-aa/f16c": (_generator("f16c", **AA), (2, 64, 64), {}, {"blur_folded": 3}),
    "generator-aa/f16x3": (_generator("f16x3", **AA), (2, 64, 64), {}, {"blur_folded": 3}),
    "embedder/resnet101@4x128": (R101, (4, 128, 128), {}, {"shortcuts_folded": 1}),
    "embedder/vgg16@4x128": (VGG, (4, 128, 128), {}, {"pools_fused": 1}),
    "embedder/resnet101@4x256": (R101, (4, 256, 256), {}, {"direct_stem": 1, "pools_fused": 1}),
    "block/C256": (B256, (4, 128, 128), {}, {"bottlenecks_fused": 2}),
    "block/C256/bneck=0": (B256, (4, 128, 128), {"GDT_CONV_BNECK": "0"}, {}),
    "block/projection": (PROJ, (4, 128, 128), {}, {"bottlenecks_fused": 1}),
    "block/projection/bneck=0": (PROJ, (4, 128, 128), {"GDT_CONV_BNECK": "0"}, {}),
    "block/projection-s2": (PROJ_S2, (2, 64, 64), {}, {"shortcuts_folded": 1}),
    "block/C1024@16x64x64": (B1024, (16, 64, 64), {}, {"conv3x3_expand": 3, "chained_reduce": 2}),
    "block/C1024@16x64x64/chain=0": (B1024, (16, 64, 64), {"GDT_XEXP_CHAIN": "0"}, {"conv3x3_expand": 3}),
    "block/C1024@16x64x64/xexp=0": (B1024, (16, 64, 64), {"GDT_CONV_XEXP": "0"}, {}),
    "block/C1024@18x64x60": (B1024, (18, 64, 60), {}, {"conv3x3_expand": 3, "chained_reduce": 2}),
    "block/C1024@18x64x60/chain=0": (B1024, (18, 64, 60), {"GDT_XEXP_CHAIN": "0"}, {"conv3x3_expand": 3}),
    "embedder/resnet18/basic=2": (R18, (2, 160, 192), BASIC, {"basic": 2}),
    "head/regional-gem-whiten": (_embedder(_head_state, head=("gem", True, 3, 1e-6, False, True)), (2, 160, 224), {}, {"head_launches": 8}),
    "head/attention-max": (_embedder(_head_state, head=("gem", False, 0, 1e-6, False, False), attention=("l2norm", True)), (2, 160, 224), {}, {"attention_launches": 2}),
    "head/median": (_embedder(_head_state, head=("geometric_median", 3, False, True)), (2, 160, 224), {}, {"head_launches": 11}),
    "head/median-attention": (_embedder(_head_state, head=("geometric_median", 3, False, False), attention=("l2norm", True)), (2, 160, 224), {}, {"attention_launches": 2}),
    "head/local": (_embedder(_head_state, head=("local", 1e-6, True)), (2, 96, 128), {}, {"head_launches": 2}),
}


_BUILT = {}


def built(make, dev=DEV, finalize=False):
    """the net of a builder, made once per process (planning-only and finalized apart)"""
    key = (make, str(dev), finalize)
    if key not in _BUILT:
        _BUILT[key] = make(dev, finalize) if finalize else make()
    return _BUILT[key]


def counters(net, n, h, w):
    """everything the plan queries tell about a geometry's decisions, as one dict"""
    blur = net.blur_summary(n, h, w)
    return dict(net.plan_summary(n, h, w), basic=net.basic_blocks_fused(n, h, w), blur_launches=blur["launches"], blur_folded=blur["folded"])


def assert_routes(label, got, least):
    for name, v in least.items():
        assert got[name] >= v, (label, name, got[name], v)


def probe(net, x, scale, fill, guard=GUARD, host=True):
    """One forward of ``net`` on (x, scale) in a workspace this function makes: ``guard`` bytes, the planned size, ``guard`` bytes -- all of it ``fill`` before the
    forward -- with outputs that hold NaN before the forward.  Returns (the outputs on the CPU, whether both guard bands still hold ``fill``); ``host`` False
    leaves the outputs on the device (a gigabyte of taps is compared there in a fraction of the time its copy takes).  A HIP error ends the whole session:
    nothing further is started on a device that has faulted."""
    assert guard % 256 == 0 and guard > 0
    lv = net._level(x, scale)
    need, shapes = net._geometry(lv.n, lv.rh, lv.rw)
    with torch.cuda.device(net.device):
        buf = torch.full((need + 2 * guard,), fill, dtype=torch.uint8, device=net.device)
        outs = [torch.full(s, float("nan"), dtype=torch.float32, device=net.device) for s in shapes]
        try:
            net._launch(*lv, buf[guard:guard + need], outs)
            torch.cuda.synchronize(net.device)
            intact = bool((buf[:guard] == fill).all()) and bool((buf[guard + need:] == fill).all())
            host = [o.cpu() for o in outs] if host else outs
        except RuntimeError as e:
            if str(e).startswith("gandtr_hip error 3:"):        # GDT_ERR_WORKSPACE: the library refused the size before any launch -- a failure, not a fault
                raise
            pytest.exit("HIP error in a probed forward, nothing further is run on this device: %s" % (e,), returncode=3)
    return host, intact


def same_bits(a, b):
    """two lists of fp32 tensors equal bit for bit (a NaN equals the same NaN)"""
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
