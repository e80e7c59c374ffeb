"""dev: compares the gfx950 code objects of two builds, kernel by kernel -- the proof of a refactor that must not change code generation
    python tools/kernel_diff.py <build A> <build B>        each a directory of .o files (one unit per .hip file) or a .so (units in link order)
Per unit it prints the kernels whose normalised disassembly or resource metadata differ (every kernel with -v) and one summary line; exit status 1
when anything differs or a kernel exists on one side only.  The disassembly is compared without addresses, encodings, comments, the alignment
padding after a function and the per-translation-unit __hip_cuid_* symbol; the metadata compared is the VGPR / AGPR / SGPR counts, LDS and scratch
size, the spill counts and the kernarg size.  It diffs two builds and nothing else.  Needs the ROCm LLVM tools (ROCM_PATH, default /opt/rocm)."""
import os, re, subprocess, sys, tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
META = {"vgpr_count": "vgpr", "agpr_count": "agpr", "sgpr_count": "sgpr", "group_segment_fixed_size": "lds", "private_segment_fixed_size": "scratch",
        "vgpr_spill_count": "vspill", "sgpr_spill_count": "sspill", "kernarg_segment_size": "kernarg"}


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def code_objects(path, tmp):
    """[(unit name, gfx950 code object file)] of a directory of .o files or of one .so"""
    if os.path.isdir(path):
        files = [(f[:-2], os.path.join(path, f)) for f in sorted(os.listdir(path)) if f.endswith(".o")]
    else:
        files = [(None, path)]
    out = []
    for unit, f in files:
        fat = os.path.join(tmp, "%d.fatbin" % len(os.listdir(tmp)))
        if subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, f], capture_output=True).returncode:
            continue                                            # no device code in this object
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]         # a .so holds one bundle per translation unit, in link order
        for i, s in enumerate(starts):
            part = "%s.%d" % (fat, i)
            open(part, "wb").write(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            if TARGET not in run("clang-offload-bundler", "--list", "--type=o", "--input=" + part):
                continue
            run("clang-offload-bundler", "--unbundle", "--type=o", "--input=" + part, "--targets=" + TARGET, "--output=" + part + ".co")
            out.append((unit if unit is not None else "unit%02d" % i, part + ".co"))
    return out


def metadata(co):
    """{kernel symbol: {field: value}} from the code object's AMDGPU metadata note"""
    kernels, cur = {}, None
    for line in run("llvm-readelf", "--notes", co).split("\n"):
        m = re.match(r"^(  - |    )\.(\w+):\s*(\S*)\s*$", line)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if cur is None:
            continue
        if m.group(2) == "name":
            kernels[m.group(3)] = cur
        elif m.group(2) in META:
            cur[META[m.group(2)]] = m.group(3)
    return kernels


def disassembly(co):
    """{function symbol: [normalised instruction lines]}"""
    funcs, cur = {}, None
    for line in run("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).split("\n"):
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        line = re.sub(r"__hip_cuid_\w+", "__hip_cuid_", line.split("//")[0]).strip()
        if cur is not None and line:
            cur.append(line)
    for body in funcs.values():                                 # alignment padding behind the last instruction
        while body and re.match(r"^(s_nop 0|s_code_end)$", body[-1]):
            body.pop()
    return funcs


def main():
    args = [a for a in sys.argv[1:] if a != "-v"]
    verbose = "-v" in sys.argv[1:]
    if len(args) != 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        a, b = dict(code_objects(args[0], ta)), dict(code_objects(args[1], tb))
        total = same = 0
        bad = False
        for unit in sorted(set(a) | set(b)):
            if unit not in a or unit not in b:
                print("%-24s only in %s" % (unit, args[0] if unit in a else args[1]))
                bad = True
                continue
            ma, mb, da, db = metadata(a[unit]), metadata(b[unit]), disassembly(a[unit]), disassembly(b[unit])
            n = ok = 0
            for k in sorted(set(ma) | set(mb)):
                n += 1
                if k not in ma or k not in mb:
                    print("%-24s %s: only in %s" % (unit, k, args[0] if k in ma else args[1]))
                    continue
                asm_eq, meta_eq = da.get(k) == db.get(k), ma[k] == mb[k]
                ok += asm_eq and meta_eq
                if verbose or not (asm_eq and meta_eq):
                    print("%-24s %s: disassembly %s (%d / %d lines), metadata %s" % (unit, k, "equal" if asm_eq else "DIFFERS", len(da.get(k, [])),
                                                                                    len(db.get(k, [])), "equal" if meta_eq else "DIFFERS"))
                    if not meta_eq:
                        print("%-24s     %s" % ("", "  ".join("%s %s -> %s" % (f, ma[k].get(f), mb[k].get(f)) for f in META.values() if ma[k].get(f) != mb[k].get(f))))
            helpers = sorted(f for f in set(da) | set(db) if f not in ma and f not in mb and da.get(f) != db.get(f))
            for f in helpers:
                print("%-24s %s (not a kernel): disassembly DIFFERS" % (unit, f))
            print("%-24s %3d kernels, %3d identical in disassembly and metadata" % (unit, n, ok))
            total += n
            same += ok
            bad |= ok != n or bool(helpers)
        print("total: %d kernels in %d units, %d identical in disassembly and metadata" % (total, len(set(a) | set(b)), same))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
