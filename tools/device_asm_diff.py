#!/usr/bin/env python3
"""Are the kernels of two builds the same device code?  A textual comparison of device assembly listings, keyed by kernel symbol.

    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S csrc/unit.hip -o unit.s        (one listing per unit, before and after)
    python tools/device_asm_diff.py --old before/*.s --new after/*.s [--count k_stencil_gen,k_stencil_mfma]

Each listing is cut into one block per kernel: from the function's label to its .Lfunc_end (the body and the .amdhsa_kernel descriptor
behind it) and the .set lines with its resource figures.
What depends only on where a function sits in its unit is normalised: the function number in .LBB<n>_<m> labels (and in the comments that name them, with their padding), .Lfunc_begin / .Lfunc_end /
.Ltmp numbers, the unit's __hip_cuid_ symbol, and .ident / .file lines.  Prints the symbols that differ, are missing or are extra, and the
kernel counts per name given with --count; exit status 0 only when both sets are equal and every block is identical text."""
import argparse
import re
import sys

NORMALISE = [
    (re.compile(r"\.LBB\d+_"), ".LBB#_"),
    (re.compile(r"\bBB\d+_"), "BB#_"),   # the same labels as the loop comments name them
    (re.compile(r"[ \t]+;"), " ;"),       # the padding in front of a comment follows the label's width
    (re.compile(r"\.Lfunc_(begin|end)\d+"), r".Lfunc_\1#"),
    (re.compile(r"\.Ltmp\d+"), ".Ltmp#"),
    (re.compile(r"__hip_cuid_\w+"), "__hip_cuid_#"),
]
SKIP = re.compile(r"^\s*\.(ident|file)\b")


def kernel_blocks(path):
    """{kernel symbol: normalised text of its body and descriptor}"""
    lines = open(path, errors="replace").read().split("\n")
    kernels = set(m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m)
    blocks = {k: [] for k in kernels}
    cur = None
    for l in lines:
        if SKIP.match(l):
            continue
        label = re.match(r"^([A-Za-z_][\w$.]*):", l)
        if cur is None and label and label.group(1) in kernels:
            cur = label.group(1)
        if cur is None:
            m = re.match(r"\s*\.set\s+([A-Za-z_][\w$]*)\.\w+,", l)   # the resource figures behind a function: .set <symbol>.num_vgpr, ...
            if m and m.group(1) in kernels:
                blocks[m.group(1)].append(l)
            continue
        for pat, rep in NORMALISE:
            l = pat.sub(rep, l)
        blocks[cur].append(l)
        if re.match(r"\s*\.Lfunc_end#:", l):
            cur = None
    return {k: "\n".join(v) for k, v in blocks.items()}


def collect(paths):
    out = {}
    for p in paths:
        for k, v in kernel_blocks(p).items():
            if k in out:
                sys.exit("kernel %s is defined in more than one listing" % k)
            out[k] = v
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--count", default="", help="comma-separated name fragments: print how many kernel symbols contain each")
    a = ap.parse_args()
    old, new = collect(a.old), collect(a.new)
    for frag in [f for f in a.count.split(",") if f]:
        print("%-24s old %4d  new %4d" % (frag, sum(frag in k for k in old), sum(frag in k for k in new)))
    missing, extra = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(k for k in set(old) & set(new) if old[k] != new[k])
    print("kernels: old %d, new %d; missing %d, extra %d, differ %d" % (len(old), len(new), len(missing), len(extra), len(differ)))
    for title, names in (("missing", missing), ("extra", extra), ("differ", differ)):
        for k in names:
            print("%s: %s" % (title, k))
    if not (missing or extra or differ):
        print("identical")
    return 1 if (missing or extra or differ) else 0


if __name__ == "__main__":
    sys.exit(main())
