"""A graph forward does not depend on what its workspace held before, writes no byte outside it and writes every output element (the contract next to
gdt_net_forward in include/gandtr_hip.h) -- and the liveness-based layout of Planner::layout() computes what a layout without any reuse computes.

Per case (net x precision x geometry x knob setting) six forwards through workspace_probe.probe: the workspace filled with 0x00, 0xFF (NaN as fp16 and fp32) and
0x7B (61280 / 1.3e36: large and finite) under GDT_PLAN_NO_REUSE=1 -- every tensor, slab and scratch block on bytes of its own -- and with the knob unset:

  A. no reuse: the three fills give the same bits; every output element is finite (the outputs hold NaN before the forward); both guard bands are untouched.
     A difference or a NaN means a launch read bytes no launch of this forward wrote, or left an output element unwritten.
  B. default layout: the three fills give the same bits, and they are A's -- kernels, routes and summation orders are the same (asserted: the plan counters), so a
     difference is a tensor released too early or two live blocks that overlap; guards untouched.
  C. the public forward, on the engine's own workspace after forwards at two other geometries, gives A's bits.

No tolerance anywhere: bit equality, finiteness, an untouched guard.  The cases are the smallest shapes at which each route is planned, confirmed per case with the
plan counters (tests/test_workspace_layout_host.py checks the same table without a device).  Each case prints its counters and its two workspace sizes."""
import math

import pytest
import torch

import workspace_probe as wp
from gandtr_amd.tools import synth
from test_plan_routes_host import NETS

pytestmark = pytest.mark.gpu


def _family(label):
    return lambda dev, finalize: NETS[label][0]().finalize()


_FAMILY_BUILDERS = {label: _family(label) for label in NETS}
CASES = {"%s@%dx%dx%d" % ((label,) + g): (_FAMILY_BUILDERS[label], g, {}, {}) for label in NETS for g in ((2, 64, 64), (1, 96, 160))}
CASES.update(wp.EXTRA)


def _input(net, n, h, w, dev):
    return synth.synth_input(11, (n, net.in_channels, h, w), 1.0).to(dev)


def _first_difference(got, want):
    """where two output lists differ: (slot, differing elements, first flat index, the two values), or None"""
    for slot, (a, b) in enumerate(zip(got, want)):
        d = (a.view(torch.int32) != b.view(torch.int32)).flatten()
        if bool(d.any()):
            i = int(d.nonzero()[0])
            return slot, int(d.sum()), i, float(a.flatten()[i]), float(b.flatten()[i])
    return None


HOST_LIMIT = 64 << 20          # bytes of outputs per forward up to which they are compared on the CPU


def _fills(net, x, scale, want, label, problems, host):
    """the three fills of one layout: every finding goes to ``problems``; returns the first fill's outputs (the reference when ``want`` is None)"""
    first = None
    for fill in wp.FILLS:
        outs, intact = wp.probe(net, x, scale, fill, host=host)
        if not intact:
            problems.append("%s fill 0x%02X: a guard band was written" % (label, fill))
        for slot, o in enumerate(outs):
            bad = int((~torch.isfinite(o)).sum())
            if bad:
                problems.append("%s fill 0x%02X: output %d holds %d non-finite elements of %d" % (label, fill, slot, bad, o.numel()))
        ref = want if want is not None else first
        if ref is not None:
            d = _first_difference(outs, ref)
            if d is not None:
                problems.append("%s fill 0x%02X differs from %s: output %d, %d elements, first at %d: %r against %r" %
                                ((label, fill, "the no-reuse layout" if want is not None else "fill 0x00") + d))
        if first is None:
            first = outs
    return first


@pytest.mark.parametrize("label", list(CASES))
def test_forward_is_independent_of_the_workspace_content(cuda_device, label):
    make, (n, h, w), settings, least = CASES[label]
    net = wp.built(make, cuda_device, True)
    x = _input(net, n, h, w, cuda_device)
    problems = []
    with wp.knobs(dict(settings, **{wp.NO_REUSE: "1"})):
        planned = wp.counters(net, n, h, w)
        wp.assert_routes(label, planned, least)
        size_apart = net.workspace_bytes(n, h, w)
        host = 4 * sum(math.prod(s) for s in net.output_shapes(n, h, w)) <= HOST_LIMIT
        want = _fills(net, x, None, None, "A", problems, host)
    with wp.knobs(settings):
        assert wp.counters(net, n, h, w) == planned
        size = net.workspace_bytes(n, h, w)
        print("%s: workspace %d bytes, %d without reuse; planned %s" % (label, size, size_apart, {k: v for k, v in planned.items() if v}))
        assert size <= size_apart
        _fills(net, x, None, want, "B", problems, host)
        for other in ((n, h + 32, w + 32), (n, h, w + 32)):           # the engine's workspace: grown for a larger geometry, then used by another
            net.forward(_input(net, *other, cuda_device))
        got = [o.cpu() if host else o for o in net.forward(x)]
        d = _first_difference(got, want)
        if d is not None:
            problems.append("C: forward on the engine's workspace differs from the no-reuse layout: output %d, %d elements, first at %d: %r against %r" % d)
    assert not problems, (label, problems)


PYRAMID = ((None, 2 ** -0.5, 0.5), (2, 160, 224))


def test_forward_many_is_independent_of_the_side_workspaces(cuda_device):
    """a three-level pyramid of the ResNet-101 embedder through forward_many -- one side stream per level -- on side workspaces that hold each fill before the
    call: the level-by-level forward's bits, under either layout"""
    scales, (n, h, w) = PYRAMID
    net = wp.built(wp.R101, cuda_device, True)
    x = _input(net, n, h, w, cuda_device)
    levels = [(x, s) for s in scales]
    for apart in ({wp.NO_REUSE: "1"}, {}):
        with wp.knobs(apart):
            want = [[o.cpu() for o in net.forward(x, scale=s)] for s in scales]
        with wp.knobs(apart):
            # (a level's plan, and with it its size, may follow the group: four times the largest level's own need is kept by _grow whatever the group plans)
            keep = 4 * max(net.workspace_bytes(n, *net.resized_size(h, w, s)) for s in scales)
            for fill in wp.FILLS:
                net._side_pools(len(levels))
                for k in range(len(levels)):
                    net._side["ws"][k] = torch.full((keep,), fill, dtype=torch.uint8, device=cuda_device)
                seeded = [b.data_ptr() for b in net._side["ws"]]
                got = net.forward_many(levels)
                torch.cuda.synchronize(cuda_device)
                assert [b.data_ptr() for b in net._side["ws"]] == seeded, "a side workspace was replaced: the fill was not what the levels ran on"
                for k, (g, r) in enumerate(zip(got, want)):
                    g = [o.cpu() for o in g]
                    assert all(bool(torch.isfinite(o).all()) for o in g), (apart, fill, k)
                    assert _first_difference(g, r) is None, (apart, fill, k, _first_difference(g, r))
    net._side["ws"] = [None] * len(net._side["ws"])
