"""GDT_PLAN_NO_REUSE=1 is the reference layout of the graph workspace -- the arena of Planner::layout() never hands out a byte twice within a plan -- and nothing
else: for every net family of test_plan_routes_host.NETS at small, odd and mid-size geometries, and for the block / head nets of workspace_probe.EXTRA, every plan
query answers the same with the knob at 1 and unset, the workspace only grows, and the knob is live (the same handle follows it at its next plan).  The sweep is
what tests/test_hip_workspace.py runs on the device: each route that makes a launch write or read a tensor of another op is planned somewhere in it.  No GPU."""
import functools

import pytest

import workspace_probe as wp
from test_plan_routes_host import NETS, SMALL

GEOMETRIES = SMALL + ((4, 128, 128), (2, 160, 224))
ROUTE_COUNTERS = ("norms_folded", "pools_fused", "direct_stem", "shortcuts_folded", "transposed_fused", "stride2_shift", "conv4x4t_launches", "convt2x2_launches",
                  "conv3x3_cat_launches", "bottlenecks_fused", "conv3x3_expand", "chained_reduce", "basic")


def _answers(net, geometry):
    """every plan query of a geometry under the current environment, or "refused" """
    try:
        return {"plan": net.plan_summary(*geometry), "plan_resize": net.plan_summary(*geometry, resize=True), "blur": net.blur_summary(*geometry),
                "basic": net.basic_blocks_fused(*geometry), "shapes": net.output_shapes(*geometry)}, net.workspace_bytes(*geometry)
    except ValueError:
        return "refused", 0


def _compare(net, geometry, settings, label):
    """the answers of a geometry (knob unset), after the comparison with the knob at 1 and the return to the unset size on the same handle"""
    with wp.knobs(settings):
        plain, size = _answers(net, geometry)
    with wp.knobs(dict(settings, **{wp.NO_REUSE: "1"})):
        apart, size_apart = _answers(net, geometry)
    with wp.knobs(dict(settings, **{wp.NO_REUSE: "0"})):
        zero, size_zero = _answers(net, geometry)
    with wp.knobs(settings):
        again, size_again = _answers(net, geometry)
    assert apart == plain and zero == plain and again == plain, (label, geometry)
    assert size_again == size == size_zero, (label, geometry, size, size_zero, size_again)      # live: back at the old size once the knob is gone
    if plain == "refused":
        return None, 0, 0
    assert size_apart >= size, (label, geometry, size, size_apart)
    return plain, size, size_apart


@functools.lru_cache(maxsize=None)
def _family(label):
    net = NETS[label][0]()
    return {g: _compare(net, g, {}, label) for g in GEOMETRIES}


@functools.lru_cache(maxsize=None)
def _extra(label):
    make, geometry, settings, least = wp.EXTRA[label]
    return _compare(wp.built(make), geometry, settings, label)


@pytest.mark.parametrize("label", list(NETS))
def test_no_reuse_changes_the_size_and_nothing_else(label):
    planned = 0
    for geometry, (plain, size, size_apart) in _family(label).items():
        if plain is None:
            continue
        planned += 1
        if plain["plan"]["conv_launches"] > 2:       # (more than two convs: some tensor has died by the time a later one is laid out, so reuse saves bytes)
            assert size_apart > size, (label, geometry, size, size_apart)
    assert planned >= 4, label                       # only the 9 x 17 geometry is refused anywhere


@pytest.mark.parametrize("label", list(wp.EXTRA))
def test_the_extra_cases_plan_their_routes(label):
    plain, size, size_apart = _extra(label)
    assert plain is not None, label
    wp.assert_routes(label, dict(plain["plan"], basic=plain["basic"], blur_folded=plain["blur"]["folded"]), wp.EXTRA[label][3])


def test_the_sweep_plans_every_route_that_crosses_ops():
    """what keeps the device sweep from being vacuous: each counter is non-zero somewhere, with the knob unset (and so, by the tests above, with it at 1)"""
    seen = dict.fromkeys(ROUTE_COUNTERS, 0)
    plans = [plain for label in NETS for plain, _, _ in _family(label).values() if plain is not None] + [_extra(label)[0] for label in wp.EXTRA]
    for plain in plans:
        for name in ROUTE_COUNTERS:
            seen[name] += plain["basic"] if name == "basic" else plain["plan"][name]
    assert all(v > 0 for v in seen.values()), seen
    assert any(p["blur"]["folded"] > 0 for p in plans)


def test_the_knob_is_one_of_the_live_knobs():
    from gandtr_amd import _hip
    assert wp.NO_REUSE in _hip.plan_knobs()
