"""Offline check of the chunk-body layout of conv3x3_halo_c16.hip ("per-MFMA layout"): the file is compiled to gfx950
assembly with the Makefile's flags, once, and tools/mfma_gaps.py reads what sits between the MFMAs.  Needs hipcc, no GPU; the compilation
takes a minute or two.

The yardstick is the row layout this one replaced (a patch row's four MFMAs back to back, then the row's companion work in one piece).  The
kernel file no longer holds it -- commit `2b4e7c4` does, as the first of two selectable layouts -- so its figures are constants here: ROW_LAYOUT below, what
this test printed for that build at that commit (same compiler, same flags), as recorded in profiles/c16_sched_gaps.txt and in the table
of DESIGN.md "per-MFMA layout".

Held: per chunk the per-MFMA layout exposes at most a QUARTER of the issue cycles the row layout exposes, in the same MODE.  The bound is
not a measurement of the new code: a chunk's 1728 MFMAs offer 1728 x 12 = 20.7 k shadow cycles, about twice the ~10-12 k issue cycles of
everything else, so an even spread exposes nothing; the quarter is the margin for waits the compiler places and for the first and last
rows of a chunk.  Also held: no MFMA -> MFMA gap of 12 or more instructions, no scratch access and no branch inside the span, no more
spilled registers than the row layout (all of them outside the loop), and the kernel still at 256 VGPRs + 256 AGPRs."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gandtr_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
MODES = (0, 1, 3, 5, 7)               # every fold mode the file instantiates
# the row layout at commit 2b4e7c4, per MODE: profiles/c16_sched_gaps.txt, DESIGN.md "per-MFMA layout"
ROW_LAYOUT = {0: {"exposed_cycles": 4717, "vgpr_spill_count": 128}, 1: {"exposed_cycles": 5373, "vgpr_spill_count": 57},
              3: {"exposed_cycles": 5918, "vgpr_spill_count": 56}, 5: {"exposed_cycles": 5458, "vgpr_spill_count": 56},
              7: {"exposed_cycles": 6057, "vgpr_spill_count": 54}}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


def _gaps():
    spec = importlib.util.spec_from_file_location("mfma_gaps", os.path.join(ROOT, "tools", "mfma_gaps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _makefile_flags():
    """the Makefile's compile line for conv3x3_halo_c16.o, with -c replaced by --cuda-device-only -S"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    base = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1)
    extra = re.search(r"^conv3x3_halo_c16\.o:\s*CXXFLAGS\s*\+=\s*(.*)$", text, re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    return (base + " " + extra).replace("$(ARCH)", arch).split()


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """{mode: figures of the first-MFMA .. last-MFMA span + metadata} of the kernel file as it is"""
    out = str(tmp_path_factory.mktemp("c16_layout") / "c16.s")
    gaps = _gaps()
    p = subprocess.run([HIPCC] + _makefile_flags() + ["--cuda-device-only", "-S", "conv3x3_halo_c16.hip", "-o", out], cwd=CSRC,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    text = open(out).read()
    res = {}
    for mode in MODES:
        (name, body), = gaps.kernels(text, r"conv3x3_halo_c16_kernelILi%dE" % mode)
        r = gaps.analyse(body)
        # the kernel's record of the amdhsa.kernels metadata: a YAML list item ("  - .key: ...") holding its .name
        meta, = [m for m in re.split(r"\n  - (?=\.)", text[text.index("amdhsa.kernels:"):]) if re.search(r"\.name:\s+%s\n" % re.escape(name), m)]
        for key in ("vgpr_spill_count", "vgpr_count", "agpr_count", "sgpr_spill_count"):
            r[key] = int(re.search(r"\.%s:\s*(\d+)" % key, meta).group(1))
        res[mode] = r
        print("MODE %d: exposed %d of %d issue cycles (row layout: %d), largest gap %d, gaps >= 12: %d, scratch %d, branches %d, VGPR spills %d (row layout: %d)"
              % (mode, r["exposed_cycles"], r["issue_cycles"], ROW_LAYOUT[mode]["exposed_cycles"], r["largest_gap"], r["gaps_ge12"], r["scratch"], r["branches"],
                 r["vgpr_spill_count"], ROW_LAYOUT[mode]["vgpr_spill_count"]))
    return res


@pytest.mark.parametrize("mode", MODES)
def test_chunk_body_is_straight_line_and_spread(layout, mode):
    r = layout[mode]
    assert r["mfma"] == 1728                               # 9 taps x (2 x 64 fp16 + 64 MX): the whole chunk body, unrolled
    assert r["gaps_ge12"] == 0 and r["largest_gap"] < 12, r["hist"]
    assert r["scratch"] == 0
    assert r["branches"] == 0


@pytest.mark.parametrize("mode", (1, 5, 7))
def test_exposed_cycles_at_most_a_quarter_of_the_row_layout(layout, mode):
    assert 4 * layout[mode]["exposed_cycles"] <= ROW_LAYOUT[mode]["exposed_cycles"], (layout[mode]["exposed_cycles"], ROW_LAYOUT[mode]["exposed_cycles"])


@pytest.mark.parametrize("mode", MODES)
def test_registers(layout, mode):
    new, old = layout[mode], ROW_LAYOUT[mode]
    assert new["vgpr_spill_count"] <= old["vgpr_spill_count"]
    assert new["vgpr_count"] == 512 and new["agpr_count"] == 256          # 256 VGPRs + 256 AGPRs of the unified file


def test_mfma_gaps_model():
    """the tool's issue model on a hand-made listing: 4 cycles per VALU / LDS / vector-memory instruction, s_nop n = n + 1, other scalar 1, 12 covered"""
    gaps = _gaps()
    body = ["s_mov_b32 s0, 0", "v_mfma_f32_16x16x32_f16 a[0:3], v[0:3], v[4:7], a[0:3]", "v_add_u32_e32 v1, v2, v3", "ds_read_b128 v[0:3], v9",
            "global_load_dwordx4 v[4:7], v8, s[0:1]", "s_nop 3", "s_waitcnt lgkmcnt(0)", "v_mfma_f32_16x16x32_f16 a[0:3], v[0:3], v[4:7], a[0:3]",
            "v_mfma_scale_f32_16x16x128_f8f6f4 a[0:3], v[0:5], v[6:9], a[0:3], v10, v11", "scratch_load_dword v1, off, s0", "s_cbranch_scc1 .LBB0_1",
            "v_mfma_f32_16x16x32_f16 a[0:3], v[0:3], v[4:7], a[0:3]", "v_mov_b32_e32 v0, 0"]
    r = gaps.analyse(body)
    assert r["mfma"] == 4 and r["hist"] == {0: 1, 2: 1, 5: 1} and r["largest_gap"] == 5 and r["empty_gaps"] == 1
    assert r["classes"] == {"valu": 1, "lds": 1, "vmem": 2, "scalar": 3}
    assert r["scratch"] == 1 and r["branches"] == 1
    assert r["issue_cycles"] == (4 + 4 + 4 + 4 + 1) + (4 + 1) and r["exposed_cycles"] == 17 - 12
    assert gaps.analyse(body, shadow=28)["exposed_cycles"] == 0
    assert gaps.analyse(["v_add_u32_e32 v1, v2, v3"]) is None
