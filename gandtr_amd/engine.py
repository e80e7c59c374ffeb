"""Host-side driver of the HIP graph executor (C ABI: include/gandtr_hip.h, binding: gandtr_amd/_hip.py).

``HipNet`` mirrors the builder calls; the ``build_*`` functions translate the reference's state dicts
(names as produced by the reference modules, see gandtr_amd/tools/synth.py) into layer graphs:

  build_generator   ResnetGenerator            mdir/components/model/network/p2p_networks.py:269-313, :454-506
  build_embedder    ImageRetrievalNet          mdir/external/cirtorch/networks/imageretrievalnet.py:101-123, :185-190
  build_hed         HedInterpolation           mdir/components/model/network/hed.py:30-83
  build_rcf         RCF                        mdir/components/model/network/rcf.py:28-155
  build_p2p_unet    P2pUNet and its four kin   mdir/components/model/network/unet.py:48-350

PyTorch is used for device memory and streams only; no torch op runs on the data path.
"""
import collections
import contextlib
import ctypes
import math
import os

import numpy as np
import torch

from . import _hip
from ._hip import ConvDesc


def _f32(t):
    """host fp32 contiguous numpy view of a tensor / array (None passes through)"""
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        t = t.detach().to("cpu", torch.float32).contiguous().numpy()
    return np.ascontiguousarray(t, dtype=np.float32)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


_SIDE_STREAMS = {}


def side_stream(device, k):
    """The k-th side stream of ``device``, shared by every net of the process.  torch hands out streams from a pool of 32 per device round-robin and the ROCm runtime
    multiplexes them onto a few hardware queues (four by default): the first net of a process got pool streams that sit on queues of their own, the third net's
    landed on the queue of the DEFAULT stream -- its pyramid levels then queued behind each other and every launch cost the host twice as much (measured: the
    same batch-1 multi-scale loop at 360 descriptors/s in a fresh process and 205 after two other networks had run in it).  One list per device keeps every net
    on the same first streams."""
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    pool = _SIDE_STREAMS.setdefault(key, [])
    while len(pool) <= k:
        pool.append(torch.cuda.Stream(device=dev))
    return pool[k]


def _stream(t):
    """the caller's stream on ``t``'s device, as the handle the C ABI takes"""
    return torch.cuda.current_stream(t.device).cuda_stream


def _out_ptrs(outs):
    return (ctypes.c_void_p * max(1, len(outs)))(*[o.data_ptr() for o in outs])


def _grow(slots, k, need, device):
    """``slots[k]``: a scratch buffer of at least ``need`` bytes (the old one is dropped BEFORE the larger one is allocated)"""
    if slots[k] is None or slots[k].numel() < need:
        slots[k] = None
        slots[k] = torch.empty(need, dtype=torch.uint8, device=device)
    return slots[k]


# one prepared level of a forward: the fp32 contiguous input on the net's device, its geometry, the resized geometry and the pack kernel's step
_Level = collections.namedtuple("_Level", "x n h w rh rw rscale")


class HipNet:
    """One layer graph living on one GPU.  Host calls are serialised per handle (one thread at a time; see forward_many for what may overlap on the device)."""

    PRECISIONS = {"f16": 0, "f16x3": 1, "f16c": 2, "f16ch": 3}       # include/gandtr_hip.h, gdt_net_set_precision

    def __init__(self, device, precision="f16"):
        self.lib = _hip.load()
        if precision not in self.PRECISIONS:
            raise ValueError("precision must be one of %s" % sorted(self.PRECISIONS))
        self.precision = precision
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("HipNet needs a cuda (HIP) device, got %s" % self.device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.handle = ctypes.c_void_p()
        _hip.check(self.lib.gdt_net_create(ctypes.byref(self.handle)))
        _hip.check(self.lib.gdt_net_set_precision(self.handle, self.PRECISIONS[precision]))
        self.in_channels = None                    # channels of the graph's input (input())
        self.out_slot = None                       # external output of the model's result (set by the build_* functions)
        self.tap_slots = {}                        # generator: tap index -> external output
        self.feature_slot = None                   # embedder: external output of the feature map, if tapped
        self.attention_slot = None                 # embedder with the local head: external output of the positions' attention
        self._finalized = False                    # finalize() ran: weights are on the device, forwards allowed, geometries cached
        self._profiling = False                    # set_profiling: per-op events; profiled forwards run eagerly, level by level
        self._group_factor = 1.0                   # the planner hint the handle holds (set_group_factor)
        self._geo_cache = {}                       # (n, rh, rw, group factor, live knobs) -> (workspace bytes, output shapes)
        self._ws = [None]                          # scratch buffer of forward() (one slot, see _grow)
        self._side = {"streams": [], "ws": []}     # per level of forward_many: side stream and scratch buffer
        self.side_workspace_cap = 8 << 30          # bytes of side scratch kept between forward_many calls

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value and self.lib is not None:
            try:
                self.lib.gdt_net_destroy(h)
            except Exception:       # interpreter shutdown: ctypes may already be torn down
                pass
            self.handle = None

    # ---- builder -------------------------------------------------------------------------------------------------
    def _add(self, op, *args):
        """call the adder ``gdt_net_<op>`` (handle first, new tensor id last) and return that id"""
        out = ctypes.c_int()
        _hip.check(getattr(self.lib, "gdt_net_" + op)(self.handle, *args, ctypes.byref(out)))
        return out.value

    def input(self, channels, perm=None, scale=None, shift=None):
        perm_a = (ctypes.c_int * channels)(*perm) if perm is not None else None
        scale_a = (ctypes.c_float * channels)(*scale) if scale is not None else None
        shift_a = (ctypes.c_float * channels)(*shift) if shift is not None else None
        out = self._add("input", channels, perm_a, scale_a, shift_a)
        self.in_channels = channels
        return out

    def input_filter(self, kind, w, p, beta, tau, eps):
        """gdt_net_input_filter: ``kind`` "edgefilter" = EdgeFilter(w, p, beta, tau, eps) applied by the input pack in fp32 (``tau`` is clamped into
        [0.01, 0.9] by the library, as EdgeFilter.forward clamps its parameter)"""
        if kind != "edgefilter":
            raise NotImplementedError("input filter %r: only 'edgefilter' is on the HIP path" % (kind,))
        _hip.check(self.lib.gdt_net_input_filter(self.handle, 1, float(w), float(p), float(beta), float(tau), float(eps)))

    def _conv(self, a, b, w, bias, bn, residual=-1, **desc):
        """gdt_net_conv of ``a`` (and ``b``, -1: none) with the fp32 weight array ``w``: the descriptor from the weight's shape and ``desc``, one gdt_conv_weights"""
        transposed = desc.get("transposed", 0)
        cin, cout = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
        d = ConvDesc(cin=cin, cout=cout, kh=w.shape[2], kw=w.shape[3], bn_eps=1e-5, **desc)
        arrays = [w, _f32(bias)] + ([_f32(t) for t in bn] if bn is not None else [None] * 4)      # (alive until the call has returned)
        return self._add("conv", a, b, ctypes.byref(d), ctypes.byref(_hip.ConvWeights(*[_ptr(t) for t in arrays])), residual)

    def conv(self, x, weight, bias=None, bn=None, stride=1, pad=0, reflect=False, transposed=False, relu=False,
             residual=-1, out_f32=False, act=0, dilation=1, leaky=0.0):
        """``leaky``: slope of an nn.LeakyReLU applied after bias and BatchNorm in place of ``relu``; ``dilation`` != 1: plain Conv2d + bias"""
        if dilation != 1 and (bn is not None or residual != -1):
            raise ValueError("a dilated conv takes no BatchNorm and no residual")
        if leaky and (dilation != 1 or residual != -1 or relu):
            raise ValueError("a LeakyReLU conv takes no dilation, no residual and no ReLU")
        return self._conv(x, -1, _f32(weight), bias, bn, residual, stride=stride, pad=pad, pad_reflect=reflect, transposed=transposed, relu=relu,
                          out_f32_nchw=out_f32, act=act, dilation=dilation, leaky=leaky)

    def conv_transposed4(self, a, weight, b=-1, relu_a=False, bias=None, bn=None, relu=False, out_f32=False, act=0):
        """nn.ConvTranspose2d(k4, s2, p1) of ``torch.cat([a, b], 1)`` (``b`` = -1: of ``a`` alone) with ReLU applied to ``a`` as it is read when ``relu_a``
        (gdt_net_conv, transposed-4 route); ``weight`` [cin_a + cin_b][cout][4][4]"""
        w = _f32(weight)
        if w.ndim != 4 or w.shape[2:] != (4, 4):
            raise ValueError("conv_transposed4 takes a [cin][cout][4][4] weight, got %s" % (tuple(w.shape),))
        return self._conv(a, b, w, bias, bn, stride=2, pad=1, transposed=1, relu=relu, out_f32_nchw=out_f32, act=act, in_relu=relu_a)

    def conv_transposed2(self, x, weight, bias=None, bn=None, relu=False):
        """nn.ConvTranspose2d(k2, s2, p0) of ``x`` (gdt_net_conv, transposed-2 route); ``weight`` [cin][cout][2][2]; internal output of 2H x 2W"""
        w = _f32(weight)
        if w.ndim != 4 or w.shape[2:] != (2, 2):
            raise ValueError("conv_transposed2 takes a [cin][cout][2][2] weight, got %s" % (tuple(w.shape),))
        return self._conv(x, -1, w, bias, bn, stride=2, pad=0, transposed=1, relu=relu)

    def conv_cat(self, a, b, weight, bias=None, bn=None, stride=1, pad=0, relu=False, out_f32=False, act=0):
        """nn.Conv2d of ``torch.cat([a, b], 1)`` (gdt_net_conv with two inputs); ``weight`` [cout][cin_a + cin_b][kh][kw], ``a``'s channels first"""
        w = _f32(weight)
        if w.ndim != 4:
            raise ValueError("conv_cat takes a [cout][cin][kh][kw] weight, got %s" % (tuple(w.shape),))
        return self._conv(a, b, w, bias, bn, stride=stride, pad=pad, relu=relu, out_f32_nchw=out_f32, act=act)

    def instance_norm(self, x, relu=False, residual=-1, eps=1e-5, leaky=0.0):
        """``leaky``: slope of an nn.LeakyReLU behind the norm in place of ``relu``"""
        if leaky and (relu or residual != -1):
            raise ValueError("a LeakyReLU InstanceNorm takes no ReLU and no residual")
        return self._add("instance_norm", x, eps, int(relu), float(leaky), residual)

    def maxpool(self, x, kernel, stride, pad=0, ceil=False):
        if ceil and pad:
            raise ValueError("ceil-mode max-pooling takes no padding here")
        return self._add("maxpool", x, kernel, stride, pad, int(ceil))

    RESIZE_MODES = {"bilinear": 0, "nearest": 1}                     # include/gandtr_hip.h, gdt_net_resize

    def resize(self, x, like, mode="bilinear"):
        """gdt_net_resize: ``F.interpolate(x, size=<the H x W of tensor like>, mode=mode)`` (bilinear: align_corners=False)"""
        if mode not in self.RESIZE_MODES:
            raise NotImplementedError("resize mode %r: only 'bilinear' and 'nearest' are on the HIP path" % (mode,))
        return self._add("resize", x, like, self.RESIZE_MODES[mode])

    def blur_resample(self, x, up=False):
        """gdt_net_blur_resample: the anti-aliased Downsample (reflect pad, [1, 2, 1] x [1, 2, 1] / 16 at stride 2) or, ``up``, Upsample (bilinear x 2) of
        CUT's ResnetGenerator.  An InstanceNorm (+ReLU) whose only consumer is this op is applied by it (``blur_summary``)."""
        return self._add("blur_resample", x, int(bool(up)))

    def gem_l2n(self, x, p, eps_gem=1e-6, eps_l2=1e-6):
        return self._add("gem_l2n", x, float(p), eps_gem, eps_l2)

    POOL_KINDS = {"mac": 0, "spoc": 1, "gem": 2, "gemmp": 3}         # include/gandtr_hip.h, gdt_net_pool_head

    def _pool_head(self, x, kind, p, eps, aggregate, levels, rwhiten, whiten, eps_l2, attention=0, normalize_max=False):
        arrays = [_f32(p).reshape(-1) if p is not None else None] + [_f32(t) for t in tuple(rwhiten or (None, None)) + tuple(whiten or (None, None))]
        pa, rw, rb, fw, fb = (_ptr(t) for t in arrays)                 # (the arrays stay alive until the call has returned)
        d = _hip.PoolHeadDesc(self.POOL_KINDS[kind], pa, 0 if arrays[0] is None else arrays[0].size, float(eps), int(aggregate), int(levels), rw, rb, fw, fb,
                              float(eps_l2), attention, int(bool(normalize_max)))
        return self._add("pool_head", x, ctypes.byref(d))

    def pool_head(self, x, kind, p=None, eps=1e-6, aggregate=0, levels=3, rwhiten=None, whiten=None, eps_l2=1e-6):
        """gdt_net_pool_head: pooling ``kind`` (global, ``aggregate`` 1 = R-MAC, 2 = regional over ``levels`` levels) -> l2n -> optional final
        whitening + l2n; ``rwhiten`` / ``whiten`` = (weight [D][D], bias [D]) of the nn.Linear layers or None"""
        return self._pool_head(x, kind, p, eps, aggregate, levels, rwhiten, whiten, eps_l2)

    def pool_head_attention(self, x, kind, normalize_max, p=None, eps=1e-6, aggregate=0, levels=3, rwhiten=None, eps_l2=1e-6):
        """gdt_net_pool_head with attention 1: ``pool_head`` (no final whitening) of the map weighted per position by its L2-norm attention, divided by the
        image's maximum when ``normalize_max``"""
        return self._pool_head(x, kind, p, eps, aggregate, levels, rwhiten, None, eps_l2, attention=1, normalize_max=normalize_max)

    def median_head(self, x, iterations, whiten=None, eps_l2=1e-6, attention=None):
        """gdt_net_median_head: geometric median of the map's positions by ``iterations`` Weiszfeld steps -> l2n -> optional final whitening + l2n
        (``whiten`` = (weight [D][D], bias [D]) or None).  ``attention`` ("l2norm", normalize_max): the median of the map weighted per position by its
        L2-norm attention (CirRetrievalNetAttention with this pooling); no whitening then"""
        if attention is not None and attention[0] != "l2norm":
            raise NotImplementedError("attention %r: only 'l2norm' is on the HIP path" % (attention[0],))
        arrays = [_f32(t) for t in tuple(whiten or (None, None))]
        fw, fb = (_ptr(t) for t in arrays)                             # (the arrays stay alive until the call has returned)
        d = _hip.MedianHeadDesc(int(iterations), fw, fb, float(eps_l2), 0 if attention is None else 1, int(bool(attention and attention[1])))
        return self._add("median_head", x, ctypes.byref(d))

    def local_head(self, x, eps=1e-6, normalize_max=False):
        """gdt_net_local_head: the map's positions as L2-normalised descriptors [N][D][H W] (returned slot) and their L2-norm attention [N][H W]
        (returned slot + 1), divided by the image's maximum when ``normalize_max``"""
        return self._add("local_head", x, float(eps), int(bool(normalize_max)))

    def output_nchw(self, x, bias=None):
        b = _f32(bias)
        return self._add("output_nchw", x, _ptr(b))

    def hed_head(self, feats, score_w, score_b, fusion_w, fusion_b, sigmoid=True):
        ws = [_f32(w).reshape(-1) for w in score_w]
        wp = (ctypes.c_void_p * 5)(*[w.ctypes.data for w in ws])
        return self._add("hed_head", (ctypes.c_int * 5)(*feats), wp, (ctypes.c_float * 5)(*[float(b) for b in score_b]),
                         (ctypes.c_float * 5)(*[float(w) for w in fusion_w]), float(fusion_b), int(sigmoid))

    def rcf_head(self, feats, stage_of, side_w, stage_b, fuse_w, fuse_b, sigmoid=True):
        """gdt_net_rcf_head: 13 feature tensors, their stages, the folded side vectors (one per feature) and stage biases"""
        if len(feats) != 13 or len(stage_of) != 13 or len(side_w) != 13 or len(stage_b) != 5 or len(fuse_w) != 5:
            raise ValueError("the RCF head takes 13 features (and stages / side vectors) and 5 stage biases / fusion weights")
        ws = [_f32(w).reshape(-1) for w in side_w]
        wp = (ctypes.c_void_p * 13)(*[w.ctypes.data for w in ws])
        return self._add("rcf_head", (ctypes.c_int * 13)(*feats), (ctypes.c_int * 13)(*stage_of), wp,
                         (ctypes.c_float * 5)(*[float(b) for b in stage_b]), (ctypes.c_float * 5)(*[float(w) for w in fuse_w]), float(fuse_b),
                         int(sigmoid))

    def finalize(self):
        with torch.cuda.device(self.device):
            _hip.check(self.lib.gdt_net_finalize(self.handle))
        self._finalized = True
        return self

    # ---- planning ------------------------------------------------------------------------------------------------
    @staticmethod
    def resized_size(h, w, scale):
        """Output size of F.interpolate(scale_factor=s): floor(float(in * s)) (torch/nn/functional.py)."""
        if scale is None:
            return h, w
        return int(math.floor(float(h * scale))), int(math.floor(float(w * scale)))

    def _geometry(self, n, rh, rw):
        """(workspace bytes, output shapes) of a geometry, planned once: every query plans the whole graph (make_plan, csrc/net_plan.hip: ~0.1 ms for ResNet-101), and a
        forward asks three times per pyramid level -- 1.2 ms of the 8.6 ms a synchronised multi-scale call took (round 5)."""
        # (the knobs the library reads every time it plans, A/B inside one process, are part of the key: the library names them itself)
        key = (n, rh, rw, self._group_factor) + tuple(os.environ.get(k) for k in _hip.plan_knobs())
        hit = self._geo_cache.get(key)
        if hit is None:
            b = ctypes.c_size_t()
            _hip.check(self.lib.gdt_net_workspace_bytes(self.handle, n, rh, rw, ctypes.byref(b)))
            shapes = []
            dims, ndim = (ctypes.c_int * 4)(), ctypes.c_int()
            for slot in range(self.lib.gdt_net_num_outputs(self.handle)):
                _hip.check(self.lib.gdt_net_output_shape(self.handle, slot, n, rh, rw, dims, ctypes.byref(ndim)))
                shapes.append(tuple(dims[i] for i in range(ndim.value)))
            if len(self._geo_cache) > 256:
                self._geo_cache.clear()
            hit = (b.value, shapes)
            if self._finalized:
                self._geo_cache[key] = hit
        return hit

    def workspace_bytes(self, n, rh, rw):
        return self._geometry(n, rh, rw)[0]

    def output_shapes(self, n, rh, rw):
        return list(self._geometry(n, rh, rw)[1])

    PLAN_KEYS = property(lambda self: _hip.plan_count_names())       # gdt_plan_count_name: one name per counter of gdt_net_plan_summary

    def plan_summary(self, n, rh, rw, resize=False):
        """the planner's decisions for a geometry as a dict of named counts (GDT_PLAN_* in include/gandtr_hip.h): host logic, no device call"""
        keys = self.PLAN_KEYS + _hip.plan_count_more_names()
        c = (ctypes.c_int * len(keys))()
        _hip.check(self.lib.gdt_net_plan_summary(self.handle, n, rh, rw, int(bool(resize)), c, len(c)))
        return dict(zip(keys, c))

    def blur_summary(self, n, rh, rw):
        """the planner's decisions about the net's blur-resample ops for a geometry: {"launches": their launches, "folded": those that apply their
        producer's InstanceNorm themselves} (gdt_net_blur_summary): host logic, no device call"""
        launches, folded = ctypes.c_int(), ctypes.c_int()
        _hip.check(self.lib.gdt_net_blur_summary(self.handle, n, rh, rw, ctypes.byref(launches), ctypes.byref(folded)))
        return {"launches": launches.value, "folded": folded.value}

    def basic_blocks_fused(self, n, rh, rw):
        """identity BasicBlocks of a geometry that run as one launch of conv3x3_basic.hip (gdt_net_basic_summary; GDT_CONV_BASIC: unset = the measured
        default, off; 0 never; 1 with enough patches; 2 wherever the shapes fit): host logic, no device call"""
        fused = ctypes.c_int()
        _hip.check(self.lib.gdt_net_basic_summary(self.handle, n, rh, rw, ctypes.byref(fused)))
        return fused.value

    def convt2x2_launches(self, n, rh, rw):
        """transposed 2x2 convs of a geometry that run as one launch of convt2x2.hip (GDT_CONVT2X2=0: none) -- the planner's count"""
        return self.plan_summary(n, rh, rw)["convt2x2_launches"]

    def conv4x4_launches(self, n, rh, rw):
        """conv launches of a geometry that run on the 4x4 patch kernel (conv4x4_halo.hip; GDT_CONV4X4_HALO=0: none) -- the planner's count"""
        return self.plan_summary(n, rh, rw)["conv4x4_launches"]

    def conv4x4t_launches(self, n, rh, rw):
        """transposed 4x4 convs of a geometry that run as one launch of conv4x4t_halo.hip (GDT_CONV4X4T_HALO=0: none) -- the planner's count"""
        return self.plan_summary(n, rh, rw)["conv4x4t_launches"]

    def conv3x3_cat_launches(self, n, rh, rw):
        """convs of a concatenation of a geometry that run as one launch of conv3x3_cat_halo.hip (GDT_CONV3X3_CAT_HALO=0: none) -- the planner's count"""
        return self.plan_summary(n, rh, rw)["conv3x3_cat_launches"]

    def head_launches(self, n, rh, rw):
        """(launches of the net's pool-head ops, launches among them that read the feature map) for a geometry -- the planner's count"""
        s = self.plan_summary(n, rh, rw)
        return s["head_launches"], s["head_map_reads"]

    def attention_launches(self, n, rh, rw):
        """(launches the attention of the net's pool-head ops adds in front of the pooling, launches of such heads that read the feature map: the norm
        pass and the weighted pooling pass) for a geometry -- the planner's count"""
        s = self.plan_summary(n, rh, rw)
        return s["attention_launches"], s["attention_map_reads"]

    def flops(self, n, rh, rw):
        f = ctypes.c_double()
        _hip.check(self.lib.gdt_net_flops(self.handle, n, rh, rw, ctypes.byref(f)))
        return f.value

    def set_group_factor(self, factor):
        """planner hint for the geometry planned next: it runs concurrently with others of this net; factor = (pixels of all of them) / (its own), 1 = alone
        (gdt_net_set_group_factor).  forward_many sets it per level and resets it."""
        factor = max(1.0, float(factor))
        if factor != self._group_factor:
            _hip.check(self.lib.gdt_net_set_group_factor(self.handle, factor))
            self._group_factor = factor

    # ---- profiling -----------------------------------------------------------------------------------------------
    def set_profiling(self, enable):
        self._profiling = bool(enable)          # profiled forwards run eagerly (events are recorded per op)
        _hip.check(self.lib.gdt_net_set_profiling(self.handle, int(enable)))

    def _profile_columns(self, read, *types):
        """the per-op columns a gdt_net_profile_read* call fills, one list per ctypes type, cut to the ops of the last profiled forward"""
        cap = max(1, int(self.lib.gdt_net_num_ops(self.handle)))
        n = ctypes.c_int()
        cols = [(t * cap)() for t in types]
        _hip.check(read(self.handle, cap, ctypes.byref(n), *cols))
        return [c[:n.value] for c in cols]

    def profile(self):
        """per-op (kind, conv N-tile, ms, algorithmic flops) of the last profiled forward"""
        return list(zip(*self._profile_columns(self.lib.gdt_net_profile_read, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double)))

    def profile_bytes(self):
        """per-op algorithmic HBM bytes of the last profiled forward (same op order as profile())"""
        return self._profile_columns(self.lib.gdt_net_profile_read_bytes, ctypes.c_double)[0]

    # ---- execution -----------------------------------------------------------------------------------------------
    def _level(self, x, scale):
        """``(x, scale)`` checked and prepared: the input as fp32, contiguous, on this net's device, and the geometry gdt_net_forward takes"""
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError("expected an N x %s x H x W input, got %s" % (self.in_channels, tuple(x.shape)))
        x = x.to(self.device).contiguous().float()
        n, _, h, w = x.shape
        rh, rw = self.resized_size(h, w, scale)
        return _Level(x, n, h, w, rh, rw, float(np.float32(1.0 / scale)) if scale is not None else 1.0)

    def _buffers(self, slots, k, lv):
        """(scratch buffer ``slots[k]`` grown to the level's need, its freshly allocated outputs), on the current stream; the geometry comes from the cache"""
        need, shapes = self._geometry(lv.n, lv.rh, lv.rw)
        return _grow(slots, k, need, self.device), self._alloc_outputs(shapes)

    def _alloc_outputs(self, shapes):
        return [torch.empty(s, dtype=torch.float32, device=self.device) for s in shapes]

    def _launch(self, x, n, h, w, rh, rw, rscale, ws, outs):
        _hip.check(self.lib.gdt_net_forward(self.handle, x.data_ptr(), n, h, w, rh, rw, rscale, _out_ptrs(outs), len(outs),
                                            ws.data_ptr(), ws.numel(), _stream(x)))

    def forward(self, x, scale=None):
        """x: fp32 NCHW tensor on this net's device.  ``scale``: optional F.interpolate scale_factor applied to the
        input inside the pack kernel.  Returns the list of external outputs (torch tensors on the device)."""
        if not self._finalized:
            raise RuntimeError("HipNet.forward before finalize()")
        lv = self._level(x, scale)
        with torch.cuda.device(self.device):
            ws, outs = self._buffers(self._ws, 0, lv)
            self._launch(*lv, ws, outs)
        return outs

    # ---- several levels in flight --------------------------------------------------------------------------------
    def _group_px(self, inputs):
        """resized pixels of a group of levels (what is not an image is refused later, level by level)"""
        return float(sum(x.shape[0] * math.prod(self.resized_size(x.shape[2], x.shape[3], s)) for x, s in inputs if x.dim() == 4))

    def _set_level_factor(self, group_px, lv):
        """Tell the planner that ``lv`` runs together with its group: fusion thresholds count the group's patches."""
        self.set_group_factor(round(group_px / float(lv.n * lv.rh * lv.rw), 3))

    def _side_pools(self, count):
        streams, slots = self._side["streams"], self._side["ws"]
        while len(streams) < count:
            streams.append(side_stream(self.device, len(streams)))
            slots.append(None)

    def _release_side_over_cap(self, cur):
        slots = self._side["ws"]
        if sum(w.numel() for w in slots if w is not None) > self.side_workspace_cap:
            for k, w in enumerate(slots):
                if w is not None:
                    w.record_stream(cur)
                    slots[k] = None

    @contextlib.contextmanager
    def _level_group(self, count):
        """The frame of a forward_many call, yielding the caller's stream: ``count`` side streams and scratch slots exist; when the body is through, the side
        scratch over ``side_workspace_cap`` is released (the caller's stream is the last to have used it); however it ends -- also when a level is refused
        half-way -- the handle is back at group factor 1, so that the next plan is a single geometry's."""
        cur = torch.cuda.current_stream(self.device)
        self._side_pools(count)
        try:
            with torch.cuda.device(self.device):
                yield cur
                self._release_side_over_cap(cur)
        finally:
            self.set_group_factor(1.0)

    def forward_many(self, inputs):
        """Several independent forwards -- ``inputs`` = [(x, scale or None), ...], e.g. the levels of the multi-scale pyramid
        (CirMultiscaleAggregation, wrapper.py:225-263) -- issued on one side stream each, every one with its own scratch buffer, and joined
        on the caller's stream.  A level at batch 8 leaves most of the chip idle (layer3 of ResNet-101 at scale 1/2: 32 patch tiles for
        256 CUs); the levels' kernels fill each other's gaps.  Results are those of ``forward`` called level by level.

        Invariant this relies on (and the C handle states, include/gandtr_hip.h): the HOST calls on one ``gdt_net`` are serialised -- each
        ``gdt_net_forward`` plans its geometry into the handle and enqueues its launches before it returns -- and every byte of per-forward
        DEVICE state lives in the caller's workspace, so several forwards of one handle may be in flight on different streams as long as each
        has its own workspace and they are issued from one host thread at a time.  The side workspaces are kept between calls up to
        ``side_workspace_cap`` bytes in total (default 8 GiB); beyond it they are released when the call returns."""
        if not self._finalized:
            raise RuntimeError("HipNet.forward_many before finalize()")
        if len(inputs) == 1 or self._profiling or os.environ.get("GANDTR_HIP_CONCURRENT_LEVELS", "1") == "0":
            return [self.forward(x, scale=s) for x, s in inputs]
        # (the order in which the host enqueues the levels -- as given, smallest first, largest first -- makes no difference: hub scales at 8 x 1024^2 6.36 / 6.56 /
        # 6.43 ms, {1, 1/sqrt 2, sqrt 2} 13.68 / 13.64 / 13.67 ms)
        results = [None] * len(inputs)
        group_px = self._group_px(inputs)
        with self._level_group(len(inputs)) as cur:
            streams = self._side["streams"]
            for k in range(len(inputs)):
                lv = self._level(*inputs[k])
                self._set_level_factor(group_px, lv)
                streams[k].wait_stream(cur)
                with torch.cuda.stream(streams[k]):
                    ws, results[k] = self._buffers(self._side["ws"], k, lv)
                    self._launch(*lv, ws, results[k])
                    lv.x.record_stream(streams[k])
            for k in range(len(inputs)):
                cur.wait_stream(streams[k])
                for o in results[k]:
                    o.record_stream(cur)
        return results

# ======================================================================================================= builders

def _bn(sd, p):
    return (sd[p + ".weight"], sd[p + ".bias"], sd[p + ".running_mean"], sd[p + ".running_var"])


def _norm_type(norm, key_norm):
    """the norm type a builder runs: the module's configured one when the caller knows it (get_norm_layer, p2p_networks.py:23-35), else the one the
    state-dict keys show"""
    norm = norm or key_norm
    if norm not in ("instance", "batch"):
        raise NotImplementedError('normalization layer [%s] is not found' % norm)          # p2p_networks.py:34
    if norm == "batch" and key_norm != "batch":
        raise NotImplementedError("BatchNorm without running statistics (track_running_stats=False) has no inference form on the HIP path")
    return norm


def _check_inorm_width(width, what):
    if width & (width - 1) or width > 2048:
        raise NotImplementedError("InstanceNorm on the HIP path needs a power-of-two channel count <= 2048: %s gives a layer of %d channels" % (what, width))


def _open(device, precision, channels=3, perm=None, in_affine=None):
    """(a new HipNet, its input tensor): ``perm`` / ``in_affine`` = (scale, shift) per channel are applied by the input pack kernel"""
    net = HipNet(device, precision)
    scale, shift = in_affine if in_affine is not None else (None, None)
    return net, net.input(channels, perm=perm, scale=scale, shift=shift)


def generator_antialias(sd):
    """(no_antialias, no_antialias_up) of a ResnetGenerator state dict: CUT's sampling layers carry a ``filt`` buffer -- a Downsample at index 7 (behind
    the first down layer's conv, norm, ReLU), an Upsample right behind the blocks"""
    no_antialias = "model.7.filt" not in sd
    n_blocks = sum(1 for k in sd if k.endswith(".conv_block.1.weight"))
    first_up = (10 if no_antialias else 12) + n_blocks
    return no_antialias, "model.%d.filt" % first_up not in sd


def generator_layout(sd):
    """(norm, ngf, n_blocks, in_nc, out_nc) recovered from state-dict keys: BatchNorm iff ``model.2.running_mean`` is
    present (use_bias rule p2p_networks.py:264-267).  The head's index follows from the sampling layers present (generator_antialias)."""
    norm = "batch" if "model.2.running_mean" in sd else "instance"
    n_blocks = sum(1 for k in sd if k.endswith(".conv_block.1.weight"))
    w0 = sd["model.1.weight"]
    no_antialias, no_antialias_up = generator_antialias(sd)
    last = (10 if no_antialias else 12) + n_blocks + (6 if no_antialias_up else 8) + 1
    return norm, w0.shape[0], n_blocks, w0.shape[1], sd["model.%d.weight" % last].shape[0]


def build_generator(sd, device, taps=(), pre_tanh=False, in_affine=None, precision="f16c", finalize=True, norm=None, stop_after_taps=False):
    """ResnetGenerator as a HIP graph.  External outputs: [generator output] + one per requested tap (in ``taps``
    order).  Taps follow the reference's nn.Sequential indices (p2p_networks.py:316-334); a norm-layer tap aliases the
    post-ReLU tensor because the reference's ReLUs are in-place (:272).  Tap 0 / the second reflection pad are not
    materialised on the device (padding is resolved inside the conv loader) and are not available.

    The layout follows the state dict (``generator_antialias``): with CUT's anti-aliased sampling a down layer is a stride-1 conv + norm + ReLU and a
    ``blur_resample`` op (Downsample), an up layer a ``blur_resample(up=True)`` op (Upsample) and a stride-1 conv + norm + ReLU; a tap on a sampling
    layer's index is the op's output.  The planner folds the InstanceNorm in front of a sampling op into it unless that norm (or its ReLU) is tapped.

    ``stop_after_taps``: the encoder-only graph (``forward(.., encode_only=True)``, p2p_networks.py:328-329) -- the graph ends with the op that
    materialises the last requested tap; there is no generator output (``out_slot`` is None).  A tapped tensor is written by its own op before any later
    layer reads it, so the ops up to there are planned as in the full graph and the taps are the full graph's, bit for bit."""
    key_norm, ngf, n_blocks, in_nc, out_nc = generator_layout(sd)
    inorm = _norm_type(norm, key_norm) == "instance"
    net, x = _open(device, precision, in_nc, in_affine=in_affine)
    tap_slots = {}

    def tap(idx, t, bias=None):
        if idx in taps and idx not in tap_slots:
            tap_slots[idx] = net.output_nchw(t, bias)

    def close(out):
        if finalize:
            net.finalize()
        net.out_slot = out
        net.tap_slots = tap_slots
        return net

    if stop_after_taps and not taps:
        raise ValueError("an encoder-only graph needs at least one tap")
    encoded = lambda: stop_after_taps and all(t in tap_slots for t in taps)

    def conv_norm_relu(x, key, nkey, idx, relu=True, residual=-1, **kw):
        """conv -> norm -> (ReLU) (+ residual).  InstanceNorm: bias-free conv (the bias cancels in the norm) + separate
        norm kernels; BatchNorm: folded into the conv epilogue."""
        if inorm:
            raw = net.conv(x, sd[key + ".weight"], None, **kw)
            if idx is not None:
                tap(idx, raw, sd.get(key + ".bias"))
            return net.instance_norm(raw, relu=relu, residual=residual)
        if idx is not None and idx in taps:   # raw conv output requested: unfused variant
            raw = net.conv(x, sd[key + ".weight"], sd.get(key + ".bias"), **kw)
            tap(idx, raw)
        return net.conv(x, sd[key + ".weight"], sd.get(key + ".bias"), bn=_bn(sd, nkey), relu=relu, residual=residual, **kw)

    h = conv_norm_relu(x, "model.1", "model.2", 1, pad=3, reflect=True)
    tap(2, h); tap(3, h)
    if encoded():
        return close(None)
    no_antialias, no_antialias_up = generator_antialias(sd)
    i = 4
    for _ in range(2):
        h = conv_norm_relu(h, "model.%d" % i, "model.%d" % (i + 1), i, stride=2 if no_antialias else 1, pad=1)
        tap(i + 1, h); tap(i + 2, h)
        if encoded():
            return close(None)
        i += 3
        if not no_antialias:      # Downsample: applies the norm in front of it itself unless that norm is tapped (Planner::norm_folds)
            h = net.blur_resample(h)
            tap(i, h)
            if encoded():
                return close(None)
            i += 1
    for _ in range(n_blocks):
        p = "model.%d.conv_block." % i
        r = conv_norm_relu(h, p + "1", p + "2", None, pad=1, reflect=True)
        h = conv_norm_relu(r, p + "5", p + "6", None, relu=False, residual=h, pad=1, reflect=True)
        tap(i, h)
        if encoded():
            return close(None)
        i += 1
    for _ in range(2):
        if no_antialias_up:
            h = conv_norm_relu(h, "model.%d" % i, "model.%d" % (i + 1), i, transposed=True, stride=2, pad=1)
        else:                     # Upsample, then a stride-1 conv
            h = net.blur_resample(h, up=True)
            tap(i, h)
            if encoded():
                return close(None)
            i += 1
            h = conv_norm_relu(h, "model.%d" % i, "model.%d" % (i + 1), i, pad=1)
        tap(i + 1, h); tap(i + 2, h)
        if encoded():
            return close(None)
        i += 3
    head = "model.%d" % (i + 1)
    if (i + 1) in taps and not pre_tanh:
        tap_slots[i + 1] = net.conv(h, sd[head + ".weight"], sd[head + ".bias"], pad=3, reflect=True, out_f32=True, act=0)
    out = net.conv(h, sd[head + ".weight"], sd[head + ".bias"], pad=3, reflect=True, out_f32=True, act=0 if pre_tanh else 1)
    if (i + 2) in taps:
        tap_slots[i + 2] = out
    return close(out)


VGG16_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512]


def _vgg16_trunk(net, x, sd, prefix="features."):
    i = 0
    for v in VGG16_CFG:
        if v == "M":
            x = net.maxpool(x, 2, 2)
            i += 1
        else:
            x = net.conv(x, sd["%s%d.weight" % (prefix, i)], sd["%s%d.bias" % (prefix, i)], pad=1, relu=True)
            i += 2
    return x


def _resnet_trunk(net, x, sd, prefix="features."):
    blocks = []
    for li in range(4):
        nb = 0
        while "%s%d.%d.conv1.weight" % (prefix, 4 + li, nb) in sd:
            nb += 1
        blocks.append(nb)
    x = net.conv(x, sd[prefix + "0.weight"], None, bn=_bn(sd, prefix + "1"), stride=2, pad=3, relu=True)
    x = net.maxpool(x, 3, 2, 1)
    for li, nb in enumerate(blocks):
        for b in range(nb):
            p = "%s%d.%d." % (prefix, 4 + li, b)
            stride = 2 if (b == 0 and li > 0) else 1
            idt = x
            if p + "downsample.0.weight" in sd:              # (every first block of a Bottleneck stage; of a BasicBlock stage only where stride or width change)
                idt = net.conv(x, sd[p + "downsample.0.weight"], None, bn=_bn(sd, p + "downsample.1"), stride=stride)
            if p + "conv3.weight" not in sd:                 # BasicBlock (resnet18 / 34): two 3x3 convs, the stride on the first
                o = net.conv(x, sd[p + "conv1.weight"], None, bn=_bn(sd, p + "bn1"), stride=stride, pad=1, relu=True)
                x = net.conv(o, sd[p + "conv2.weight"], None, bn=_bn(sd, p + "bn2"), pad=1, relu=True, residual=idt)
                continue
            o = net.conv(x, sd[p + "conv1.weight"], None, bn=_bn(sd, p + "bn1"), relu=True)
            o = net.conv(o, sd[p + "conv2.weight"], None, bn=_bn(sd, p + "bn2"), stride=stride, pad=1, relu=True)
            x = net.conv(o, sd[p + "conv3.weight"], None, bn=_bn(sd, p + "bn3"), relu=True, residual=idt)
    return x


def embedder_arch(sd):
    """'vgg16' or 'resnet101'-style trunk, recognised from the state-dict keys (imageretrievalnet.py:185-190)."""
    return "resnet" if "features.4.0.conv1.weight" in sd else "vgg16"


def build_embedder(sd, device, in_affine=None, feature_tap=False, precision="f16", finalize=True, head=None, attention=None, preprocessing=None):
    """ImageRetrievalNet.forward as a HIP graph.  External output 0: descriptors as a row-major [N][D] fp32 matrix (the reference returns its
    transpose view, D x N).

    ``head`` None: the hub configuration -- GeM, no whitening layers (lwhiten=None, whiten=None) -- on its own op (gem_l2n).  Otherwise the tuple
    ``ImageRetrievalNet._hip_head`` gives: (pooling "mac" | "spoc" | "gem" | "gemmp" | "rmac", regional, L, eps of the pooling, local whitening, final
    whitening); the layers' weights are the reference's state-dict entries (``lwhiten.*``, ``pool.p`` / ``pool.rpool.p``, ``pool.whiten.*``,
    ``whiten.*``).  The local whitening is a 1x1 conv with bias and no ReLU in front of the pool; everything behind the map is one pool_head op.
    ``("geometric_median", iterations, local whitening, final whitening)``: the dict-valued pooling GeometricMedianWeiszfeld, on one median_head op
    (csrc/median_pool.hip), alone or with ``attention``.

    ``attention`` ("l2norm", normalize_max): CirRetrievalNetAttention -- the map is weighted per position by its L2 norm (divided by the image's maximum
    when normalize_max) inside the pooling pass (pool_head_attention); no local and no final whitening, as the reference asserts.  With ``head`` None
    the pooling is the hub's GeM.  ``preprocessing`` ("edgefilter", w, p, beta, tau, eps): CirRetrievalNetPreprocessing -- the EdgeFilter is evaluated by
    the input pack, behind resize and ``in_affine``; p / tau None: the state dict's ``preprocessing.p`` / ``preprocessing.tau``.  The number of input
    channels is that of ``features.0.weight`` (init_cirnet_inchan: 1 or 3)."""
    channels = int(sd["features.0.weight"].shape[1])
    net, x = _open(device, precision, channels=channels, in_affine=in_affine)
    if preprocessing is not None:
        kind, fw, fp, fbeta, ftau, feps = preprocessing
        fp = float(sd["preprocessing.p"].reshape(-1)[0]) if fp is None else fp
        ftau = float(sd["preprocessing.tau"].reshape(-1)[0]) if ftau is None else ftau
        net.input_filter(kind, fw, fp, fbeta, ftau, feps)
    f = _resnet_trunk(net, x, sd) if embedder_arch(sd) == "resnet" else _vgg16_trunk(net, x, sd)
    if attention is not None and attention[0] != "l2norm":
        raise NotImplementedError("attention %r: only 'l2norm' is on the HIP path" % (attention[0],))
    if head is not None and head[0] == "local":
        # ("local", eps of the L2N layer, normalize_max): no pooling -- the local head's two outputs (descriptors, attention slot = out_slot + 1)
        if attention is not None:
            raise NotImplementedError("the local head computes the L2-norm attention itself")
        net.out_slot = net.local_head(f, head[1], head[2])
        net.attention_slot = net.out_slot + 1
    elif head is None and attention is None:
        net.out_slot = net.gem_l2n(f, float(sd["pool.p"].reshape(-1)[0]))
    elif head is not None and head[0] == "geometric_median":
        # the dict-valued pooling GeometricMedianWeiszfeld: ("geometric_median", iterations, local whitening, final whitening); no parameters of its own
        _, iterations, local_whitening, whitening = head
        if attention is not None and (local_whitening or whitening):
            raise NotImplementedError("the attention net takes no local and no final whitening (cirnet.py:117)")
        if local_whitening:
            w = sd["lwhiten.weight"]
            f = net.conv(f, w.reshape(w.shape[0], w.shape[1], 1, 1), sd["lwhiten.bias"], relu=False)
        net.out_slot = net.median_head(f, iterations, whiten=(sd["whiten.weight"], sd["whiten.bias"]) if whitening else None, attention=attention)
    else:
        kind, regional, levels, eps, local_whitening, whitening = head if head is not None else ("gem", False, 0, 1e-6, False, False)
        if attention is not None and (local_whitening or whitening):
            raise NotImplementedError("the attention net takes no local and no final whitening (cirnet.py:117)")
        if regional and kind == "rmac":
            raise NotImplementedError("regions of R-MAC regions are not on the HIP path")
        if local_whitening:
            w = sd["lwhiten.weight"]
            f = net.conv(f, w.reshape(w.shape[0], w.shape[1], 1, 1), sd["lwhiten.bias"], relu=False)
        pool = dict(p=sd.get("pool.rpool.p" if regional else "pool.p") if kind in ("gem", "gemmp") else None, eps=eps,
                    aggregate=2 if regional else (1 if kind == "rmac" else 0), levels=levels or 3,
                    rwhiten=(sd["pool.whiten.weight"], sd["pool.whiten.bias"]) if regional and "pool.whiten.weight" in sd else None)
        kind = "mac" if kind == "rmac" else kind
        if attention is not None:
            net.out_slot = net.pool_head_attention(f, kind, attention[1], **pool)
        else:
            net.out_slot = net.pool_head(f, kind, whiten=(sd["whiten.weight"], sd["whiten.bias"]) if whitening else None, **pool)
    net.feature_slot = net.output_nchw(f) if feature_tap else None
    if finalize:
        net.finalize()
    return net


def build_hed(sd, device, perm=None, in_affine=None, sigmoid=True, precision="f16", finalize=True):
    """HedInterpolation.forward (hed.py:60-83); ``perm``/``in_affine`` fold the RgbToBgrPre + MeanStdPre wrappers
    (wrapper.py:351-364, :182-194) into the input pack kernel."""
    net, x = _open(device, precision, perm=perm, in_affine=in_affine)
    feats = []
    for bi in range(5):
        off = 0
        if bi > 0:
            x = net.maxpool(x, 2, 2)
            off = 1
        ci = 0
        while "vgg%d.%d.weight" % (bi + 1, off + 2 * ci) in sd:
            k = "vgg%d.%d" % (bi + 1, off + 2 * ci)
            x = net.conv(x, sd[k + ".weight"], sd[k + ".bias"], pad=1, relu=True)
            ci += 1
        feats.append(x)
    net.out_slot = net.hed_head(
        feats, [sd["score%d.weight" % (k + 1)] for k in range(5)], [float(sd["score%d.bias" % (k + 1)]) for k in range(5)],
        [float(v) for v in sd["fusion.0.weight"].reshape(-1)], float(sd["fusion.0.bias"]), sigmoid)
    if finalize:
        net.finalize()
    return net


RCF_BLOCKS = ((64, 64), (128, 128), (256, 256, 256), (512, 512, 512), (512, 512, 512))


def rcf_fold_side(sd):
    """The linear part of RCF's side outputs folded per conv (rcf.py:115-133): conv*_down (21 x C, bias) then score_dsn (1 x 21, bias) of its stage is
    ONE C-vector W_down^T w_dsn per conv plus one constant per stage (w_dsn . sum of the stage's down biases + b_dsn), in float64.  Returns
    (stage_of [13], side vectors [13] (float64 numpy), stage biases [5])."""
    stage_of, side_w, stage_b = [], [], []
    for bi, chans in enumerate(RCF_BLOCKS):
        wd = sd["score_dsn%d.weight" % (bi + 1)].double().reshape(-1)
        bsum = sd["score_dsn%d.bias" % (bi + 1)].double().reshape(-1)[0]
        for ci in range(len(chans)):
            k = "conv%d_%d_down" % (bi + 1, ci + 1)
            w = sd[k + ".weight"].double().reshape(21, -1)
            side_w.append((w.t() @ wd).numpy())
            bsum = bsum + (wd * sd[k + ".bias"].double()).sum()
            stage_of.append(bi)
        stage_b.append(float(bsum))
    return stage_of, side_w, stage_b


def build_rcf(sd, device, perm=None, in_affine=None, sigmoid=True, precision="f16", finalize=True):
    """RCF.forward (rcf.py:100-155): the VGG trunk with ceil-mode pools (pool4 at stride 1) and dilated conv5_x, then the RCF head.  ``perm`` /
    ``in_affine`` fold the rcfngan wrapper chain (MeanStdPre, RgbToBgrPre, MeanStdPre; wrapper.py:182-194, :351-364) into the input pack; with no
    resize, in the fp16 mode, the first conv reads the caller's fp32 image itself (conv_stem.hip pair form)."""
    net, x = _open(device, precision, perm=perm, in_affine=in_affine)
    feats = []
    pools = ((2, 2), (2, 2), (2, 2), (2, 1))          # pool1-3: MaxPool2d(2, 2, ceil_mode=True); pool4: stride 1 (rcf.py:43-46)
    for bi, chans in enumerate(RCF_BLOCKS):
        if bi > 0:
            x = net.maxpool(x, pools[bi - 1][0], pools[bi - 1][1], ceil=True)
        dil = 2 if bi == 4 else 1                      # conv5_x: padding 2, dilation 2
        for ci in range(len(chans)):
            k = "conv%d_%d" % (bi + 1, ci + 1)
            x = net.conv(x, sd[k + ".weight"], sd[k + ".bias"], pad=dil, relu=True, dilation=dil)
            feats.append(x)
    stage_of, side_w, stage_b = rcf_fold_side(sd)
    net.out_slot = net.rcf_head(feats, stage_of, side_w, stage_b, [float(v) for v in sd["score_fuse.weight"].reshape(-1)],
                                float(sd["score_fuse.bias"].reshape(-1)[0]), sigmoid)
    if finalize:
        net.finalize()
    return net


def discriminator_layout(sd):
    """(norm, ndf, n_layers, in_nc) of an NLayerDiscriminator state dict: BatchNorm iff ``model.3.running_mean`` is present; the convs sit at the
    nn.Sequential indices 0, 2, 5, 8, .. (p2p_networks.py:533-563: conv + LeakyReLU, then conv + norm + LeakyReLU triples, then the 1-channel conv)"""
    convs = sorted(int(k.split(".")[1]) for k in sd if k.endswith(".weight") and sd[k].dim() == 4)
    norm = "batch" if "model.3.running_mean" in sd else "instance"
    w0 = sd["model.0.weight"]
    return norm, w0.shape[0], len(convs) - 2, w0.shape[1]


def build_discriminator(sd, device, precision="f16", finalize=True, norm=None, slope=0.2):
    """NLayerDiscriminator (p2p_networks.py:509-571, no_antialias) as a HIP graph: Conv(k4, s2, p1) + LeakyReLU, n_layers - 1 times Conv(k4, s2, p1) + norm +
    LeakyReLU, Conv(k4, s1, p1) + norm + LeakyReLU, Conv(k4, s1, p1) -> the one-channel fp32 logit map (the external output).  BatchNorm (eval) is folded into
    its conv, whose epilogue applies the LeakyReLU; InstanceNorm(affine=False) is its own op with the LeakyReLU fused (the conv's bias cancels in it)."""
    if precision not in ("f16", "f16x3"):
        raise NotImplementedError("the discriminator runs in 'f16' or 'f16x3'; %r is a generator mode" % (precision,))
    key_norm, ndf, n_layers, in_nc = discriminator_layout(sd)
    norm = _norm_type(norm, key_norm)
    net, x = _open(device, precision, in_nc)
    h = net.conv(x, sd["model.0.weight"], sd["model.0.bias"], stride=2, pad=1, leaky=slope)
    i = 2
    for layer in range(1, n_layers + 1):
        key, nkey = "model.%d" % i, "model.%d" % (i + 1)
        stride = 2 if layer < n_layers else 1
        if norm == "instance":
            _check_inorm_width(sd[key + ".weight"].shape[0], "ndf = %d" % ndf)
            h = net.instance_norm(net.conv(h, sd[key + ".weight"], None, stride=stride, pad=1), leaky=slope)
        else:
            h = net.conv(h, sd[key + ".weight"], sd.get(key + ".bias"), bn=_bn(sd, nkey), stride=stride, pad=1, leaky=slope)
        i += 3
    net.out_slot = net.conv(h, sd["model.%d.weight" % i], sd["model.%d.bias" % i], pad=1, out_f32=True, act=0)
    if finalize:
        net.finalize()
    return net


def unet_block_prefix(i):
    """state-dict prefix of the nn.Sequential of level i of a UnetGenerator: the outermost block keeps its submodule at index 1, every other block at
    index 3 (behind LeakyReLU, conv, norm).  Inside: outermost -- down conv 0, up conv 3; middle -- down conv 1, down norm 2, up conv 5, up norm 6;
    innermost -- down conv 1, up conv 3, up norm 4 (p2p_networks.py:204-230)"""
    return "model.model." + ("1.model." + "3.model." * (i - 1) if i else "")


def unet_layout(sd):
    """(norm, ngf, num_downs, in_nc, out_nc) of a UnetGenerator state dict: a level exists while its down conv does; BatchNorm iff the second level's down
    norm carries running statistics"""
    depth = 0
    while unet_block_prefix(depth + 1) + "1.weight" in sd:
        depth += 1
    w0 = sd["model.model.0.weight"]
    norm = "batch" if unet_block_prefix(1) + "2.running_mean" in sd else "instance"
    return norm, w0.shape[0], depth + 1, w0.shape[1], sd["model.model.3.weight"].shape[1]


def build_unet_generator(sd, device, precision="f16", pre_tanh=False, finalize=True, norm=None):
    """UnetGenerator (p2p_networks.py:132-236) as a HIP graph; the external output is the tanh map (``pre_tanh``: the map in front of it).

    Stored tensors.  The reference's LeakyReLU is in place, so a block hands ``cat([leaky(x), up], 1)`` to its parent, whose ReLU acts on both halves;
    relu(leaky(x)) = relu(x).  Per level i the graph therefore stores ONE down tensor s_i = leaky(d_i) (d_i the normalised down output; the next down
    conv reads it as it is, the up conv of level i reads it through ReLU-on-read) and ONE up tensor relu(u_i), which is only ever read through that ReLU.
    Down convs: BatchNorm folded + LeakyReLU in the conv epilogue, or conv + instance_norm(leaky) (the conv's bias cancels in the norm); the innermost
    has no norm and a fused ReLU (its only reader is the ReLU in front of the up conv).  Up convs: conv_transposed4 of [relu(s_i), relu(u_(i+1))]
    -- BatchNorm folded + fused ReLU, or followed by instance_norm(relu).  The outermost up conv has a bias and writes the external fp32 NCHW output.
    Dropout (eval) is the identity."""
    if precision not in ("f16", "f16x3"):
        raise NotImplementedError("the U-Net generator runs in 'f16' or 'f16x3'; %r is a ResnetGenerator mode" % (precision,))
    key_norm, ngf, num_downs, in_nc, out_nc = unet_layout(sd)
    inorm = _norm_type(norm, key_norm) == "instance"
    if inorm:
        for width in (ngf, 2 * ngf, 4 * ngf, 8 * ngf):
            _check_inorm_width(width, "ngf = %d" % ngf)
    net, x = _open(device, precision, in_nc)
    block = unet_block_prefix
    last = num_downs - 1
    # ---- down path: s[i] = the stored down tensor of level i
    s = [net.conv(x, sd[block(0) + "0.weight"], sd.get(block(0) + "0.bias"), stride=2, pad=1, leaky=0.2)]
    for i in range(1, num_downs):
        key = block(i) + "1"
        if i == last:
            s.append(net.conv(s[-1], sd[key + ".weight"], sd.get(key + ".bias"), stride=2, pad=1, relu=True))
        elif inorm:
            s.append(net.instance_norm(net.conv(s[-1], sd[key + ".weight"], None, stride=2, pad=1), leaky=0.2))
        else:
            s.append(net.conv(s[-1], sd[key + ".weight"], sd.get(key + ".bias"), bn=_bn(sd, block(i) + "2"), stride=2, pad=1, leaky=0.2))
    # ---- up path
    u = -1
    for i in range(last, 0, -1):
        key, nkey = (block(i) + "3", block(i) + "4") if i == last else (block(i) + "5", block(i) + "6")
        relu_a = i != last                       # (the innermost down tensor is stored with its ReLU applied)
        if inorm:
            u = net.instance_norm(net.conv_transposed4(s[i], sd[key + ".weight"], u, relu_a=relu_a), relu=True)
        else:
            u = net.conv_transposed4(s[i], sd[key + ".weight"], u, relu_a=relu_a, bias=sd.get(key + ".bias"), bn=_bn(sd, nkey), relu=True)
    net.out_slot = net.conv_transposed4(s[0], sd[block(0) + "3.weight"], u, relu_a=True, bias=sd[block(0) + "3.bias"], out_f32=True, act=0 if pre_tanh else 1)
    if finalize:
        net.finalize()
    return net


def p2p_unet_check(label, cfg):
    """what the device path of the normalisation U-Nets (components/model/network/unet.py) does not do, refused before anything is built"""
    co = dict(cfg["conv_opts"])
    co.pop("bias", None)
    if co != {"kernel_size": 4, "stride": 2, "padding": 1}:
        raise NotImplementedError("HIP %s runs the reference's down / up convs, kernel_size 4, stride 2, padding 1; conv_opts %r has no device form" % (label, cfg["conv_opts"]))
    if cfg["in_channels"] > 8:
        raise NotImplementedError("HIP %s takes at most 8 input channels (the input pack kernel), got %d" % (label, cfg["in_channels"]))


def build_p2p_unet(label, sd, device, cfg, precision="f16", pre_act=False, finalize=True):
    """One of the normalisation U-Nets (unet.py: ``p2p_unet``, ``outconv_unet``, ``inconv_p2p_unet``, ``aligned_p2p_unet``, ``shallow_p2p_unet``) as a HIP graph,
    built by walking the family's own layer list (``unet.family_layers(label, cfg)``; ``cfg`` from ``unet.family_config``).

    A conv takes the BatchNorm behind it (folded) and the activation behind that (epilogue) with it; Dropout is the identity.  No activation of the family is
    in place, so the stored tensors are the post-activation ones and a skip block's value is the PAIR (what the block received, what its ``nested`` chain
    returned): the layer that follows reads the concatenation from the two tensors -- a ConvTranspose2d(k4, s2, p1) through conv_transposed4, a Conv2d
    (the aligned net's Conv2d(128, 64, 3, padding=1)) through conv_cat.  The last layer writes the external fp32 NCHW output, with the Tanh where the
    net has one (``pre_act``: the map in front of it)."""
    from .components.model.network import unet
    if precision not in ("f16", "f16x3"):
        raise NotImplementedError("%s runs in 'f16' or 'f16x3'; %r is a ResnetGenerator mode" % (label, precision))
    p2p_unet_check(label, cfg)
    layers = unet.family_layers(label, cfg)
    net, x = _open(device, precision, cfg["in_channels"])

    def walk(items, prefix, value, top):
        i = 0
        while i < len(items):
            item, name = items[i], "%s%d" % (prefix, i)
            if item[0] == "skip":
                if isinstance(value, tuple):
                    raise NotImplementedError("a skip block that receives a concatenation has no device form")
                value = (value, walk(item[1], name + ".nested.", value, False))
                i += 1
                continue
            if item[0] not in ("conv", "convt"):
                raise NotImplementedError("layer %s of %s does not follow a conv" % (item[0], label))
            # ---- the conv and what rides on it: [BatchNorm] [Dropout] [activation]
            bn, relu, leaky, tanh = None, False, 0.0, False
            j = i + 1
            if j < len(items) and items[j][0] == "bn":
                key = "%s%d" % (prefix, j)
                if key + ".running_mean" not in sd:
                    raise NotImplementedError("BatchNorm without running statistics (track_running_stats=False) has no inference form on the HIP path")
                if items[j][2].get("eps", 1e-5) != 1e-5 or not items[j][2].get("affine", True):
                    raise NotImplementedError("HIP %s folds nn.BatchNorm2d(eps=1e-5, affine=True) only, got %r" % (label, items[j][2]))
                bn = _bn(sd, key)
                j += 1
            if j < len(items) and items[j][0] == "dropout":
                j += 1
            if j < len(items) and items[j][0] in ("relu", "leaky", "tanh"):
                relu, leaky, tanh = items[j][0] == "relu", items[j][1] if items[j][0] == "leaky" else 0.0, items[j][0] == "tanh"
                j += 1
            last = top and j == len(items)
            if tanh and not last:
                raise NotImplementedError("a Tanh inside the net has no device form")
            act = 1 if tanh and not pre_act else 0
            w, b = sd[name + ".weight"], sd.get(name + ".bias")
            opts = item[3]
            k, stride, pad = opts.get("kernel_size", 1), opts.get("stride", 1), opts.get("padding", 0)
            pair = isinstance(value, tuple)
            if item[0] == "convt":
                if leaky:
                    raise NotImplementedError("a LeakyReLU behind a transposed conv has no device form")
                a, second = value if pair else (value, -1)
                value = net.conv_transposed4(a, w, second, bias=b, bn=bn, relu=relu, out_f32=last, act=act)
            elif pair:
                if leaky:
                    raise NotImplementedError("a LeakyReLU behind a conv of a concatenation has no device form")
                value = net.conv_cat(value[0], value[1], w, bias=b, bn=bn, stride=stride, pad=pad, relu=relu, out_f32=last, act=act)
            else:
                value = net.conv(value, w, b, bn=bn, stride=stride, pad=pad, relu=relu, leaky=leaky, out_f32=last, act=act)
            i = j
        return value

    net.out_slot = walk(layers, "outerblock.", x, True)
    if finalize:
        net.finalize()
    return net


def orig_unet_check(cfg):
    """what the device path of ``orig_unet`` (components/model/network/unet.py, OrigUNet) does not do, refused before anything is built"""
    if cfg["min_channels"] != 64:
        raise NotImplementedError("HIP orig_unet needs min_channels = 64: its outconv is Conv2d(64, out_channels, 1) whatever min_channels is, so the forward "
                                  "of min_channels = %d fails in torch as well" % cfg["min_channels"])
    if cfg["in_channels"] > 8:
        raise NotImplementedError("HIP orig_unet takes at most 8 input channels (the input pack kernel), got %d" % cfg["in_channels"])


def build_orig_unet(sd, device, cfg, precision="f16", finalize=True):
    """``orig_unet`` (unet.py, OrigUNet) as a HIP graph.  Per skip block: the two 3x3 convs of ``downconv`` with fused ReLU -> x1; MaxPool2d(2) of x1 as its own
    op (x1 has a second reader, the skip, so the planner does not fold the pool into conv2's epilogue); the nested block; ``convT`` on the transposed-2 route
    (conv_transposed2) -> x2; ``upconv.conv1`` as the conv of the pair (x1, x2) (conv_cat: the concatenation is never written where conv3x3_cat_halo.hip takes
    the layer), ``upconv.conv2``.  ``outconv`` (1x1) writes the external fp32 NCHW output."""
    if precision not in ("f16", "f16x3"):
        raise NotImplementedError("orig_unet runs in 'f16' or 'f16x3'; %r is a ResnetGenerator mode" % (precision,))
    orig_unet_check(cfg)
    net, x = _open(device, precision, cfg["in_channels"])

    def conv_block(value, prefix, pair=None):
        w1, b1 = sd[prefix + "conv1.weight"], sd[prefix + "conv1.bias"]
        if pair is None:
            value = net.conv(value, w1, b1, pad=1, relu=True)
        else:
            value = net.conv_cat(pair[0], pair[1], w1, bias=b1, pad=1, relu=True)
        return net.conv(value, sd[prefix + "conv2.weight"], sd[prefix + "conv2.bias"], pad=1, relu=True)

    def block(value, prefix, level):
        if level == cfg["nested_levels"]:                      # the innermost conv block
            return conv_block(value, prefix)
        x1 = conv_block(value, prefix + "downconv.")
        inner = block(net.maxpool(x1, 2, 2, 0), prefix + "nested.", level + 1)
        x2 = net.conv_transposed2(inner, sd[prefix + "convT.weight"], sd[prefix + "convT.bias"])
        return conv_block(None, prefix + "upconv.", pair=(x1, x2))

    y = block(x, "outerblock.", 0)
    net.out_slot = net.conv(y, sd["outconv.weight"], sd["outconv.bias"], out_f32=True)
    if finalize:
        net.finalize()
    return net


DYNINT_CONV_OPTS = {"kernel_size": 4, "stride": 2, "padding": 1}
DYNINT_UPCONV_OPTS = {"kernel_size": 3, "stride": 1, "padding": 1}


def dynint_unet_check(cfg):
    """what the device path of ``outconv_dynint_unet`` (unet.py, OutconvP2pUNetDynamicInterpolate) does not do, refused before anything is built"""
    if cfg["upsample"] not in HipNet.RESIZE_MODES:
        raise NotImplementedError("HIP outconv_dynint_unet resizes with 'bilinear' or 'nearest'; upsample = %r has no device form" % (cfg["upsample"],))
    if cfg["conv_opts"] != DYNINT_CONV_OPTS:
        raise NotImplementedError("HIP outconv_dynint_unet runs the reference's down convs, kernel_size 4, stride 2, padding 1; conv_opts %r has no device form" % (cfg["conv_opts"],))
    if cfg["upconv_opts"] != DYNINT_UPCONV_OPTS:
        raise NotImplementedError("HIP outconv_dynint_unet runs the reference's up convs, kernel_size 3, stride 1, padding 1; upconv_opts %r has no device form" % (cfg["upconv_opts"],))
    if cfg["in_channels"] > 8:
        raise NotImplementedError("HIP outconv_dynint_unet takes at most 8 input channels (the input pack kernel), got %d" % cfg["in_channels"])
    if cfg["outconv_channels"] % 8:
        raise NotImplementedError("HIP outconv_dynint_unet needs outconv_channels %% 8 == 0 (an internal tensor), got %d" % cfg["outconv_channels"])
    if cfg["nested_levels"] < 1:
        raise NotImplementedError("HIP outconv_dynint_unet needs at least one skip block (its last up conv reads 128 channels)")


def build_dynint_unet(sd, device, cfg, precision="f16", finalize=True):
    """``outconv_dynint_unet`` (unet.py, OutconvP2pUNetDynamicInterpolate) as a HIP graph; takes ANY image size: every map is floor(H / 2) of the one above and
    is resized back to exactly the size its block received.  Per block: Conv(k4, s2, p1) [+ folded BatchNorm] + LeakyReLU(0.2) in the conv epilogue; the
    nested block; a resize (gdt_net_resize) to the block input's size; Conv(k3, s1, p1) [+ BatchNorm] + ReLU (Dropout is the identity).  A block's value is the
    PAIR (what it received, its up conv's result).  Bilinear and nearest resizing act per channel, so the two tensors of a pair are resized separately and the
    conv behind them reads the pair through conv_cat: no concatenation is written where conv3x3_cat_halo.hip takes the layer."""
    if precision not in ("f16", "f16x3"):
        raise NotImplementedError("outconv_dynint_unet runs in 'f16' or 'f16x3'; %r is a ResnetGenerator mode" % (precision,))
    dynint_unet_check(cfg)
    mode = cfg["upsample"]
    net, x = _open(device, precision, cfg["in_channels"])

    def norm(key):
        if key is None or not cfg["batchnorm"]:              # (the net's own last up conv has no BatchNorm)
            return None
        if key + ".running_mean" not in sd:
            raise NotImplementedError("BatchNorm without running statistics (track_running_stats=False) has no inference form on the HIP path")
        return _bn(sd, key)

    def up(value, like, prefix, bn_key, out_f32=False):
        """the conv at ``prefix`` + "0" (+ BatchNorm + ReLU) of ``value`` (a tensor or a pair) resized to the size of ``like``"""
        w, b = sd[prefix + "0.weight"], sd.get(prefix + "0.bias")
        if isinstance(value, tuple):
            return net.conv_cat(net.resize(value[0], like, mode), net.resize(value[1], like, mode), w, bias=b, bn=norm(bn_key), pad=1, relu=True)
        return net.conv(net.resize(value, like, mode), w, b, bn=norm(bn_key), pad=1, relu=True)

    def block(value, prefix, level):
        d = net.conv(value, sd[prefix + "down.0.weight"], sd.get(prefix + "down.0.bias"), bn=norm(prefix + "down.1"), stride=2, pad=1, leaky=0.2)
        inner = d
        if level + 1 < cfg["nested_levels"]:
            inner = block(d, "%sdown.%d." % (prefix, 3 if cfg["batchnorm"] else 2), level + 1)
        return value, up(inner, value, prefix + "up.", prefix + "up.1")

    d0 = net.conv(x, sd["down.0.weight"], sd.get("down.0.bias"), stride=2, pad=1, leaky=0.2)
    y = up(block(d0, "down.2.", 0), x, "up.", None)
    k = cfg["outconv_kernel"]
    net.out_slot = net.conv(y, sd["up.2.weight"], sd.get("up.2.bias"), pad=k // 2, out_f32=True)
    if finalize:
        net.finalize()
    return net


# ======================================================================================== stand-alone descriptor ops

def ms_aggregate(x, msp):
    """x: [S][N][D] fp32 cuda -> [N][D]  (wrapper.py:236-245, batched)."""
    lib = _hip.load()
    x = x.contiguous().float()
    s, n, d = x.shape
    y = torch.empty((n, d), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _hip.check(lib.gdt_ms_aggregate(x.data_ptr(), y.data_ptr(), s, n, d, float(msp), _stream(x)))
    return y


def whiten(v, P, m, dims=None, float64=False):
    """v: [N][D], P: [D][D], m: [D] or [D][1] (cuda) -> [N][dims]  (wrapper.py:320-322, batched).  ``float64``: the arithmetic of the
    reference's ``whiten`` stage (numpy float64, mdir/stages/whiten.py:20-23) instead of the float32 of the inference wrapper."""
    lib = _hip.load()
    dt = torch.float64 if float64 else torch.float32
    v = v.contiguous().to(dt)
    P = P.contiguous().to(dt)
    m = m.contiguous().to(dt).reshape(-1)
    n, d = v.shape
    dims = int(dims or P.shape[0])
    tmp = torch.empty((n, dims), dtype=dt, device=v.device)
    out = torch.empty((n, dims), dtype=dt, device=v.device)
    fn = lib.gdt_whiten_f64 if float64 else lib.gdt_whiten
    with torch.cuda.device(v.device):
        _hip.check(fn(P.data_ptr(), m.data_ptr(), v.data_ptr(), tmp.data_ptr(), out.data_ptr(), n, d, dims, _stream(v)))
    return out


def gem_l2n(fmap, p=3.0, eps_gem=1e-6, eps_l2=1e-6):
    """fmap: N x D x h x w fp32 cuda (reference layout).  Returns (gem N x D x 1 x 1, l2n(gem) N x D x 1 x 1):
    cirtorch layers/functional.py:21-22, :130-131."""
    lib = _hip.load()
    if not fmap.is_cuda or fmap.dim() != 4:
        raise ValueError("gem_l2n needs an N x D x h x w tensor on a HIP device")
    fmap = fmap.contiguous().float()
    n, d, h, w = fmap.shape
    pooled = torch.empty((n, d), dtype=torch.float32, device=fmap.device)
    out = torch.empty((n, d), dtype=torch.float32, device=fmap.device)
    with torch.cuda.device(fmap.device):
        _hip.check(lib.gdt_gem_l2n(fmap.data_ptr(), n, d, h, w, float(p), eps_gem, eps_l2, pooled.data_ptr(), out.data_ptr(), _stream(fmap)))
    return pooled.view(n, d, 1, 1), out.view(n, d, 1, 1)


def _nhwc_map(fmap, what):
    if not fmap.is_cuda or fmap.dim() != 4 or fmap.dtype not in (torch.float16, torch.float32):
        raise ValueError("%s needs an N x H x W x D fp16 or fp32 tensor on a HIP device" % what)
    return fmap.contiguous()


def pixel_attention(fmap, normalize_max=False):
    """gdt_pixel_attention: L2NormAttention of an NHWC map (N x H x W x D, fp16 or fp32, D % 64 == 0) per image -> fp32 N x H x W"""
    lib = _hip.load()
    fmap = _nhwc_map(fmap, "pixel_attention")
    n, h, w, d = fmap.shape
    with torch.cuda.device(fmap.device):
        need = ctypes.c_size_t()
        _hip.check(lib.gdt_pixel_attention_workspace_bytes(n, h, w, ctypes.byref(need)))
        ws = torch.empty(max(1, need.value), dtype=torch.uint8, device=fmap.device)
        out = torch.empty((n, h, w), dtype=torch.float32, device=fmap.device)
        _hip.check(lib.gdt_pixel_attention(fmap.data_ptr(), int(fmap.dtype == torch.float32), n, h, w, d, int(bool(normalize_max)), out.data_ptr(),
                                           ws.data_ptr(), ws.numel(), _stream(fmap)))
    return out


def local_descriptors(fmap, eps=1e-6, normalize_max=False):
    """gdt_local_descriptors, the local head's kernel on its own: NHWC map (fp16 or fp32, D % 64 == 0) -> (fp32 N x D x H x W descriptors
    x / (||x||_2 + eps) per position, fp32 N x H x W attention sqrt(sum x^2 + 1e-10), divided by the image's maximum when ``normalize_max``)"""
    lib = _hip.load()
    if not (fmap.is_cuda and fmap.dim() == 4 and fmap.dtype in (torch.float16, torch.float32)):
        raise ValueError("local_descriptors takes an N x H x W x D fp16 or fp32 map on a HIP device")
    fmap = fmap.contiguous()
    n, h, w, d = fmap.shape
    f32 = int(fmap.dtype == torch.float32)
    need = ctypes.c_size_t()
    _hip.check(lib.gdt_local_descriptors_workspace_bytes(n, h, w, d, f32, ctypes.byref(need)))
    with torch.cuda.device(fmap.device):
        desc = torch.empty((n, d, h, w), dtype=torch.float32, device=fmap.device)
        att = torch.empty((n, h, w), dtype=torch.float32, device=fmap.device)
        ws = torch.empty(max(need.value, 4), dtype=torch.uint8, device=fmap.device)
        _hip.check(lib.gdt_local_descriptors(fmap.data_ptr(), f32, n, h, w, d, float(eps), int(bool(normalize_max)), desc.data_ptr(), att.data_ptr(),
                                             ws.data_ptr(), ws.numel(), _stream(fmap)))
    return desc, att


def pool_regions_weighted(fmap, weights, kind, p=3.0, p_channels=None, eps=1e-6, levels=0):
    """gdt_pool_regions_weighted: the one-pass region pooling of ``fmap * weights[..., None]`` (NHWC map, fp32 N x H x W weights) -> fp32 N x R x D, R the
    boxes of gdt_rpool_regions(h, w, levels); ``kind`` as HipNet.POOL_KINDS"""
    lib = _hip.load()
    fmap = _nhwc_map(fmap, "pool_regions_weighted")
    n, h, w, d = fmap.shape
    if not weights.is_cuda or weights.dtype != torch.float32 or tuple(weights.shape) != (n, h, w):
        raise ValueError("pool_regions_weighted needs fp32 N x H x W weights on the map's device")
    weights = weights.contiguous()
    cnt = ctypes.c_int()
    _hip.check(lib.gdt_rpool_regions(h, w, levels, None, 0, ctypes.byref(cnt)))
    pc = p_channels.to(fmap.device, torch.float32).contiguous() if p_channels is not None else None
    with torch.cuda.device(fmap.device):
        out = torch.empty((n, cnt.value, d), dtype=torch.float32, device=fmap.device)
        _hip.check(lib.gdt_pool_regions_weighted(fmap.data_ptr(), int(fmap.dtype == torch.float32), n, h, w, d, HipNet.POOL_KINDS[kind], float(p),
                                                 pc.data_ptr() if pc is not None else None, float(eps), int(levels), weights.data_ptr(), out.data_ptr(),
                                                 _stream(fmap)))
    return out


def geometric_median(fmap, iterations, scale=None, prior=None):
    """gdt_geometric_median: the geometric median of the positions of each image of an NHWC map (N x H x W x D, fp16 or fp32, D % 64 == 0) by
    ``iterations`` Weiszfeld steps (0: the mean) -> fp32 N x D.  ``scale``: fp32 N x H x W, the map is taken as ``fmap * scale[..., None]``; ``prior``: fp32
    N x H x W prior weights a_i (w_i = a_i / |m - y_i|); None: ones"""
    lib = _hip.load()
    fmap = _nhwc_map(fmap, "geometric_median")
    n, h, w, d = fmap.shape
    if int(iterations) != iterations or iterations < 0:
        raise ValueError("geometric_median needs a non-negative integer number of iterations, got %r" % (iterations,))
    for name, t in (("scale", scale), ("prior", prior)):
        if t is not None and (not t.is_cuda or t.device != fmap.device or t.dtype != torch.float32 or tuple(t.shape) != (n, h, w)):
            raise ValueError("geometric_median needs fp32 N x H x W %s on the map's device" % name)
    scale = scale.contiguous() if scale is not None else None
    prior = prior.contiguous() if prior is not None else None
    with torch.cuda.device(fmap.device):
        need = ctypes.c_size_t()
        _hip.check(lib.gdt_geometric_median_workspace_bytes(n, h, w, d, ctypes.byref(need)))
        ws = torch.empty(max(1, need.value), dtype=torch.uint8, device=fmap.device)
        out = torch.empty((n, d), dtype=torch.float32, device=fmap.device)
        _hip.check(lib.gdt_geometric_median(fmap.data_ptr(), int(fmap.dtype == torch.float32), n, h, w, d, int(iterations),
                                            scale.data_ptr() if scale is not None else None, prior.data_ptr() if prior is not None else None,
                                            out.data_ptr(), ws.data_ptr(), ws.numel(), _stream(fmap)))
    return out


def pack_input_filter(x, filt, out_f32=True):
    """gdt_pack_input_filter: the input pack (fp32 NCHW -> NHWC8) with ``filt`` = ("edgefilter", w, p, beta, tau, eps) applied in fp32 in front of the rounding"""
    lib = _hip.load()
    if not x.is_cuda or x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError("pack_input_filter needs an fp32 N x C x H x W tensor on a HIP device")
    kind, fw, fp, fbeta, ftau, feps = filt
    if kind != "edgefilter":
        raise NotImplementedError("input filter %r" % (kind,))
    x = x.contiguous()
    n, c, h, w = x.shape
    with torch.cuda.device(x.device):
        out = torch.empty((n, h, w, 8), dtype=torch.float32 if out_f32 else torch.float16, device=x.device)
        _hip.check(lib.gdt_pack_input_filter(x.data_ptr(), n, c, h, w, int(bool(out_f32)), 1, float(fw), float(fp), float(fbeta), float(ftau), float(feps),
                                             out.data_ptr(), _stream(x)))
    return out


def l2n_rows(x, eps=1e-6):
    lib = _hip.load()
    x = x.contiguous().float()
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _hip.check(lib.gdt_l2n_rows(x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], eps, _stream(x)))
    return y
