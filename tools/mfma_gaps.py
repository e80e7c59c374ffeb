#!/usr/bin/env python3
"""dev: what sits between the MFMAs of a kernel, read from a `hipcc -S` listing (no GPU needed).
    python tools/mfma_gaps.py <file.s> <kernel-name regex> [--shadow CYCLES] [--json]
For every kernel whose symbol matches, over the span from its first to its last MFMA:
  * the histogram of non-MFMA instructions per MFMA -> MFMA gap, and the largest gap;
  * instruction counts by class (VALU, LDS, vector memory, scalar), and the scratch accesses and branches in the span;
  * modelled issue cycles of the non-MFMA instructions and the part of them no MFMA shadow covers.
Issue model (one wave per SIMD, in-order issue): 4 cycles per VALU / LDS / vector-memory instruction, `s_nop n` n + 1, any other scalar
instruction 1; behind every MFMA the matrix pipe is busy for SHADOW more cycles (default 12: the 16-cycle 16 x 16 shapes; 28 for the
32-cycle 32 x 32 ones), during which the wave may issue other work for free.  A gap's cost beyond the shadow is exposed.  Instructions are
classified by their mnemonic's class prefix only; waits for data (s_waitcnt) count as one scalar instruction: the model says where the
issue port is short of shadow, not how long a load takes."""
import argparse, collections, json, re, sys

CLASSES = ("valu", "lds", "vmem", "scalar")


def classify(op):
    """class of an instruction by its prefix: mfma / valu / lds / vmem / scalar"""
    if op.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_", "tbuffer_", "image_")):
        return "vmem"
    if op.startswith("v_"):
        return "valu"
    return "scalar"


def cost(ins):
    op = ins.split()[0]
    if op == "s_nop":
        return 1 + int(ins.split()[1], 0)
    return 1 if classify(op) == "scalar" else 4


def kernels(text, pattern):
    """[(symbol, [instruction lines])] of the functions whose symbol matches"""
    lines = text.split("\n")
    out = []
    for i, l in enumerate(lines):
        m = re.match(r"^([A-Za-z_][\w$.]*):", l)
        if not m or m.group(1).startswith(".L") or not re.search(pattern, m.group(1)):
            continue
        body = []
        for x in lines[i + 1:]:
            s = x.split(";")[0].split("//")[0].strip()
            if s.startswith((".Lfunc_end", ".end_amdhsa_kernel", ".section")):
                break
            if not s or s.startswith(".") or re.match(r"^\S+:$", s):
                continue
            body.append(s)
        out.append((m.group(1), body))
    return out


def analyse(body, shadow=12):
    """figures of the first-MFMA .. last-MFMA span of one kernel, or None when it holds no MFMA"""
    idx = [k for k, x in enumerate(body) if classify(x.split()[0]) == "mfma"]
    if not idx:
        return None
    gaps, cur = [], None
    for x in body[idx[0]:idx[-1] + 1]:
        if classify(x.split()[0]) == "mfma":
            if cur is not None:
                gaps.append(cur)
            cur = []
        else:
            cur.append(x)
    flat = [x for g in gaps for x in g]
    count = collections.Counter(classify(x.split()[0]) for x in flat)
    return {
        "mfma": len(idx),
        "instructions": len(flat) + len(idx),
        "hist": dict(sorted(collections.Counter(len(g) for g in gaps).items())),
        "largest_gap": max((len(g) for g in gaps), default=0),
        "gaps_ge12": sum(len(g) >= 12 for g in gaps),
        "empty_gaps": sum(not g for g in gaps),
        "classes": {c: count.get(c, 0) for c in CLASSES},
        "scratch": sum(x.split()[0].startswith("scratch_") for x in flat),
        "branches": sum(bool(re.match(r"s_c?branch|s_setpc|s_swappc|s_call", x.split()[0])) for x in flat),
        "issue_cycles": sum(cost(x) for x in flat),
        "exposed_cycles": sum(max(0, sum(cost(x) for x in g) - shadow) for g in gaps),
        "shadow": shadow,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("kernel", help="regex on the kernel symbol")
    ap.add_argument("--shadow", type=int, default=12, help="issue cycles an MFMA covers behind itself (12: 16 x 16 shapes, 28: 32 x 32)")
    ap.add_argument("--json", action="store_true", help="one JSON object per kernel instead of the table")
    a = ap.parse_args()
    found = 0
    for name, body in kernels(open(a.asm).read(), a.kernel):
        r = analyse(body, a.shadow)
        if r is None:
            continue
        found += 1
        if a.json:
            print(json.dumps(dict(r, kernel=name)))
            continue
        print(name)
        print("  span: %d instructions, %d MFMAs, %d gaps (%d empty)" % (r["instructions"], r["mfma"], r["mfma"] - 1, r["empty_gaps"]))
        print("  instructions per gap: " + "  ".join("%d:%d" % kv for kv in r["hist"].items()))
        print("  largest gap %d, gaps of >= 12 instructions: %d" % (r["largest_gap"], r["gaps_ge12"]))
        print("  classes: " + "  ".join("%s %d" % (c, r["classes"][c]) for c in CLASSES) + "; scratch accesses %d, branches %d" % (r["scratch"], r["branches"]))
        print("  issue cycles of the non-MFMA instructions %d; shadow %d x %d = %d; exposed %d (%.2f per MFMA)"
              % (r["issue_cycles"], r["mfma"], a.shadow, r["mfma"] * a.shadow, r["exposed_cycles"], r["exposed_cycles"] / r["mfma"]))
    if not found:
        sys.exit("no kernel with MFMAs matches %r" % a.kernel)


if __name__ == "__main__":
    main()
