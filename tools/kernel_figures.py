#!/usr/bin/env python3
"""Per-kernel resource figures of two builds of the library, side by side.

Both builds are made with the Makefile's flags plus
  -Rpass-analysis=kernel-resource-usage -save-temps=obj
one object per directory (DIR/<object>/<source>-hip-amdgcn-amd-amdhsa-gfx950.s). For every kernel the table
has VGPRs, SGPR and VGPR spills, scratch bytes per lane, LDS bytes per block and occupancy of both builds (the
compiler's remarks), and whether the kernel's assembly - instructions, labels, kernel descriptor; comments
stripped - is the same text.

  tools/kernel_figures.py PARENT_DIR NEW_DIR > profiles/<name>_kernel_figures.txt
Exit status 1 when a kernel of NEW has lower occupancy, more scratch or more LDS than in PARENT, or is missing.
"""
import glob
import os
import re
import subprocess
import sys

FIELDS = (("vgpr", "VGPRs"), ("sspill", "SGPRs Spill"), ("vspill", "VGPRs Spill"), ("scratch", "ScratchSize [bytes/lane]"),
          ("lds", "LDS Size [bytes/block]"), ("occ", "Occupancy [waves/SIMD]"))


def figures(path):
    """{mangled name: {field: value}} from the compiler's kernel-resource-usage remarks"""
    res, cur = {}, None
    for line in open(path):
        m = re.match(r"remark: [^ ]+ +(.+?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return {k: {f: int(v.get(r, -1)) for f, r in FIELDS} for k, v in res.items()}


def kernels(path):
    """{mangled name: instructions and directives, comments stripped} for every kernel of one device assembly file.
    Comments carry the names of IR blocks, which number differently whenever anything in the file moves; so do the
    prefixes of local labels, which are made the same."""
    out, name = {}, None
    for line in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name = m.group(1)
        line = line.split(";", 1)[0].rstrip()
        # local labels carry the function's index in the file (.LBB22_7, .Lfunc_end22) or a file-wide count
        line = re.sub(r"\.L(BB|func_begin|func_end)\d+", r".L\1", re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", line))
        if name and line:
            out.setdefault(name, []).append(line)
        if ".end_amdhsa_kernel" in line:
            name = None
    return {k: "\n".join(v) for k, v in out.items() if any(".amdhsa_kernel" in l for l in v)}


def strip_params(name):
    """a demangled function without its trailing parameter list; `(anonymous namespace)::f<...>(...)` keeps its front"""
    if not name.endswith(")"):
        return name
    depth = 0
    for i in range(len(name) - 1, -1, -1):
        depth += name[i] == ")"
        depth -= name[i] == "("
        if depth == 0:
            return name[:i]
    return name


def demangle(names):
    try:
        txt = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        short = [re.sub(r"^void ", "", strip_params(t)) for t in txt.splitlines()]
        return dict(zip(names, short))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    parent, new = sys.argv[1], sys.argv[2]
    bad = 0
    print("# Kernel resource figures of two builds of the library, parent against new: tools/kernel_figures.py PARENT_DIR NEW_DIR")
    print("# (both built with the Makefile's flags plus -Rpass-analysis=kernel-resource-usage -save-temps=obj).")
    print("# object / kernel: VGPRs, SGPR spills, VGPR spills, scratch [bytes/lane], LDS [bytes/block], occupancy [waves/SIMD];")
    print("# a -> b: parent -> new where they differ. asm same: the kernel's assembly without comments is identical text.")
    print("# WORSE marks a kernel with lower occupancy, more scratch or more LDS in the new build.")
    for d in sorted(glob.glob(os.path.join(parent, "*"))):
        obj = os.path.basename(d)
        pa = glob.glob(os.path.join(d, "*-hip-amdgcn-amd-amdhsa-gfx950.s"))
        na = glob.glob(os.path.join(new, obj, "*-hip-amdgcn-amd-amdhsa-gfx950.s"))
        if not pa or not na:
            continue
        kp, kn = kernels(pa[0]), kernels(na[0])
        fp, fn = figures(os.path.join(d, "remarks.txt")), figures(os.path.join(new, obj, "remarks.txt"))
        if not kp and not kn:
            continue
        nsame = sum(1 for k in kp if kn.get(k) == kp[k])
        # the compilation unit's id symbol is a hash of the source file's path
        whole = [[l for l in open(f) if "__hip_cuid_" not in l] for f in (pa[0], na[0])]
        print(f"\n== {obj}: {len(kp)} kernels, {nsame} with identical assembly; the file "
              f"{'is byte-identical' if whole[0] == whole[1] else 'differs'} (__hip_cuid lines apart)")
        names = demangle(sorted(set(kp) | set(kn)))
        for k in sorted(set(kp) | set(kn), key=lambda n: names[n]):
            if k not in kn or k not in kp:
                print(f"{names[k]}: only in {'parent' if k in kp else 'new'}")
                bad += 1
                continue
            a, b = fp[k], fn[k]
            worse = b["occ"] < a["occ"] or b["scratch"] > a["scratch"] or b["lds"] > a["lds"]
            bad += worse
            cols = " ".join(f"{f} {a[f]}->{b[f]}" if a[f] != b[f] else f"{f} {a[f]}" for f, _ in FIELDS)
            print(f"{names[k]}: {cols} asm {'same' if kp[k] == kn[k] else 'differs'}{'  WORSE' if worse else ''}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
