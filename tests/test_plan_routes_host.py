"""What the planner decides, net by net: the whole ``plan_summary()`` (with and without ``resize=True``), ``workspace_bytes()`` and ``output_shapes()`` of every
net family at small, odd and benchmarked geometries, with the three route knobs (GDT_CONV4X4T_HALO, GDT_CONVT2X2, GDT_CONV3X3_CAT_HALO) unset, each at 0, and the
concatenation knob at 2 -- against tests/golden/plan_routes.json.  Planning needs no device (``finalize=False``).  No GPU.

The fixture was written by ``record()`` below (``python tests/test_plan_routes_host.py --record``) run on the commit BEFORE the three routes became plan
decisions, where executor, copy op and counters each asked the eligibility predicates themselves.  It is the record of that behaviour: it is never regenerated
from the code under test.  A planner change that is meant to move a decision edits the affected entries by hand, with the reason in its commit message."""
import contextlib
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))

from gandtr_amd import engine                                   # noqa: E402
from gandtr_amd.components.model.network import unet            # noqa: E402
from gandtr_amd.tools import synth                              # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "plan_routes.json")
DEV = "cuda:0"        # only recorded; no device call happens before finalize()
ROUTE_KNOBS = ("GDT_CONV4X4T_HALO", "GDT_CONVT2X2", "GDT_CONV3X3_CAT_HALO")
KNOB_SETTINGS = {"unset": {}, "GDT_CONV4X4T_HALO=0": {"GDT_CONV4X4T_HALO": "0"}, "GDT_CONVT2X2=0": {"GDT_CONVT2X2": "0"},
                 "GDT_CONV3X3_CAT_HALO=0": {"GDT_CONV3X3_CAT_HALO": "0"}, "GDT_CONV3X3_CAT_HALO=2": {"GDT_CONV3X3_CAT_HALO": "2"}}
SMALL = ((2, 64, 64), (1, 96, 160), (2, 9, 17))
GAN_SIZE, EMBEDDER_SIZE = (64, 256, 256), (8, 1024, 1024)          # the benchmarked geometries


def _unet(norm, precision):
    return lambda: engine.build_unet_generator(synth.unet_state(0, norm, num_downs=5), DEV, precision=precision, finalize=False, norm=norm)


def _p2p(label):
    def make():
        cfg = unet.family_config(label, 3, 3, nested_levels=2)
        return engine.build_p2p_unet(label, synth.p2p_unet_state(label, 0, in_channels=3, out_channels=3, nested_levels=2), DEV, cfg, finalize=False)
    return make


def _orig(precision):
    def make():
        cfg = dict(in_channels=3, out_channels=3, nested_levels=2, min_channels=64)
        return engine.build_orig_unet(synth.orig_unet_state(0, **cfg), DEV, cfg, precision=precision, finalize=False)
    return make


def _dynint():
    model = unet.OutconvP2pUNetDynamicInterpolate(3, 3, nested_levels=2, upsample="bilinear")
    return engine.build_dynint_unet(synth.dynint_unet_state(0, in_channels=3, out_channels=3, nested_levels=2), DEV, model._cfg, finalize=False)


NETS = {
    "unet_generator/batch/f16": (_unet("batch", "f16"), GAN_SIZE),
    "unet_generator/batch/f16x3": (_unet("batch", "f16x3"), GAN_SIZE),
    "unet_generator/instance/f16": (_unet("instance", "f16"), GAN_SIZE),
    "unet_generator/instance/f16x3": (_unet("instance", "f16x3"), GAN_SIZE),
    "p2p_unet": (_p2p("p2p_unet"), GAN_SIZE),
    "aligned_p2p_unet": (_p2p("aligned_p2p_unet"), GAN_SIZE),
    "orig_unet/f16": (_orig("f16"), GAN_SIZE),
    "orig_unet/f16x3": (_orig("f16x3"), GAN_SIZE),
    "outconv_dynint_unet": (_dynint, GAN_SIZE),
    "discriminator/batch": (lambda: engine.build_discriminator(synth.discriminator_state(0, "batch"), DEV, finalize=False), GAN_SIZE),
    "discriminator/instance": (lambda: engine.build_discriminator(synth.discriminator_state(0, "instance"), DEV, finalize=False), GAN_SIZE),
    "generator/f16": (lambda: engine.build_generator(synth.generator_state(0), DEV, precision="f16", finalize=False), GAN_SIZE),
    "generator/f16c": (lambda: engine.build_generator(synth.generator_state(0), DEV, precision="f16c", finalize=False), GAN_SIZE),
    "generator/f16x3": (lambda: engine.build_generator(synth.generator_state(0), DEV, precision="f16x3", finalize=False), GAN_SIZE),
    "embedder/resnet101": (lambda: engine.build_embedder(synth.resnet101_state(0), DEV, finalize=False), EMBEDDER_SIZE),
    "embedder/vgg16": (lambda: engine.build_embedder(synth.vgg16_state(0), DEV, finalize=False), EMBEDDER_SIZE),
    "hed": (lambda: engine.build_hed(synth.hed_state(0), DEV, finalize=False), GAN_SIZE),
    "rcf": (lambda: engine.build_rcf(synth.rcf_state(0), DEV, finalize=False), GAN_SIZE),
}


@contextlib.contextmanager
def _environment(settings):
    """no GDT_* variable but ``settings`` for the duration"""
    saved = {k: v for k, v in os.environ.items() if k.startswith("GDT_")}
    for k in saved:
        del os.environ[k]
    os.environ.update(settings)
    try:
        yield
    finally:
        for k in settings:
            del os.environ[k]
        os.environ.update(saved)


def decisions(label):
    """{"n,h,w": {knob setting: entry}}; an entry is "refused" where the planner rejects the geometry (ValueError), else the counters of plan_summary() in the
    order of its keys, without and with resize, the workspace size and the output shapes"""
    make, big = NETS[label]
    net = make()
    out = {}
    for geometry in SMALL + (big,):
        per_knob = out.setdefault(",".join(str(v) for v in geometry), {})
        for name, settings in KNOB_SETTINGS.items():
            with _environment(settings):
                try:
                    plan, plan_resize = net.plan_summary(*geometry), net.plan_summary(*geometry, resize=True)
                    per_knob[name] = {"keys": list(plan), "plan": list(plan.values()), "plan_resize": [plan_resize[k] for k in plan],
                                      "workspace_bytes": net.workspace_bytes(*geometry), "output_shapes": [list(s) for s in net.output_shapes(*geometry)]}
                except ValueError:
                    per_knob[name] = "refused"
    return out


def record():
    keys = None
    nets = {}
    for label in NETS:
        nets[label] = decisions(label)
        for per_knob in nets[label].values():
            for entry in per_knob.values():
                if entry != "refused":
                    keys = keys or entry["keys"]
                    assert entry.pop("keys") == keys
        print("recorded", label, flush=True)
    with open(FIXTURE, "w") as f:
        json.dump({"plan_keys": keys, "nets": nets}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ != "__main__":
    with open(FIXTURE) as _f:
        GOLD = json.load(_f)


@pytest.mark.parametrize("label", list(NETS))
def test_planner_decisions_are_the_recorded_ones(label):
    want = GOLD["nets"][label]
    got = decisions(label)
    assert sorted(got) == sorted(want)
    for geometry, per_knob in got.items():
        assert sorted(per_knob) == sorted(want[geometry]) == sorted(KNOB_SETTINGS)
        for name, entry in per_knob.items():
            expect = want[geometry][name]
            if entry != "refused":
                assert entry.pop("keys") == GOLD["plan_keys"], (label, geometry, name)
                entry, expect = dict(entry, plan=dict(zip(GOLD["plan_keys"], entry["plan"])), plan_resize=dict(zip(GOLD["plan_keys"], entry["plan_resize"]))), \
                    dict(expect, plan=dict(zip(GOLD["plan_keys"], expect["plan"])), plan_resize=dict(zip(GOLD["plan_keys"], expect["plan_resize"])))
            assert entry == expect, (label, geometry, name)


def test_the_sweep_exercises_the_three_routes():
    """the recorded sweep is no vacuous guard: each route's counter is non-zero somewhere with the knobs unset and zero everywhere with its knob at 0, while
    the workspace size and the output shapes are the same under every knob setting"""
    keys = GOLD["plan_keys"]
    for counter, knob in (("conv4x4t_launches", "GDT_CONV4X4T_HALO"), ("convt2x2_launches", "GDT_CONVT2X2"), ("conv3x3_cat_launches", "GDT_CONV3X3_CAT_HALO")):
        k = keys.index(counter)
        entries = [per_knob for net in GOLD["nets"].values() for per_knob in net.values() if per_knob["unset"] != "refused"]
        assert any(e["unset"]["plan"][k] > 0 for e in entries), counter
        assert all(e[knob + "=0"]["plan"][k] == 0 and e[knob + "=0"]["plan_resize"][k] == 0 for e in entries), counter
    for net in GOLD["nets"].values():
        for per_knob in net.values():
            if per_knob["unset"] != "refused":
                for entry in per_knob.values():
                    assert entry["workspace_bytes"] == per_knob["unset"]["workspace_bytes"] and entry["output_shapes"] == per_knob["unset"]["output_shapes"]


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_plan_routes_host.py --record"
    record()
