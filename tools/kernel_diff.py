#!/usr/bin/env python3
"""Compare the kernels of two builds from their device assembly listings (hipcc -S, one .s per translation unit).

  tools/kernel_diff.py DIR_A DIR_B

Every *.s of a directory is split per kernel symbol: the instruction text between `<symbol>:` and its .Lfunc_end label, and the
.amdhsa_ lines of the symbol's kernel descriptor.  Comments and the compiler's local labels' numbering, which depend on where a
kernel stands in its unit, are left out.  Reported: kernels on one side only and kernels whose text or descriptor differs (a side
that emits a kernel in several units is compared by the set of versions it holds).  Exit status 1 if there is any.

Listings of a build: python -c "from lft_amd import _lib; _lib.listings('DIR')"."""
import glob
import os
import re
import sys


def kernels(directory):
    """{symbol: {unit: (text, descriptor)}} of every listing in the directory"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        unit = os.path.basename(path)[:-2]
        sym, body, desc = None, [], None          # the descriptor block stands between a kernel's last instruction and its end label
        for line in open(path, errors="replace"):
            line = line.split(";")[0].strip()
            m = re.match(r"(_Z\w+):$", line)
            if m and sym is None:
                sym, body, desc = m.group(1), [], []
            elif sym and line.startswith(".Lfunc_end"):
                out.setdefault(sym, {})[unit] = ("\n".join(body), "\n".join(desc))
                sym = None
            elif sym and line.startswith((".amdhsa_", ".end_amdhsa_")):
                desc.append(line)
            elif sym and line:
                body.append(line)
    # local labels are numbered through the unit: rename them per kernel in order of appearance
    for units in out.values():
        for u, (text, desc) in units.items():
            names = {}
            text = re.sub(r"\.L\w+", lambda m: names.setdefault(m.group(0), f".L{len(names)}"), text)
            units[u] = (text, desc)
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    for sym in sorted(set(a) - set(b)):
        print(f"only in A ({', '.join(a[sym])}): {sym}")
    for sym in sorted(set(b) - set(a)):
        print(f"only in B ({', '.join(b[sym])}): {sym}")
    bad = len(set(a) ^ set(b))
    for sym in sorted(set(a) & set(b)):
        va, vb = set(a[sym].values()), set(b[sym].values())     # a side that emits the kernel in several units may hold several versions
        if va == vb:
            continue
        bad += 1
        same = [f"A:{ua} = B:{ub}" for ua, x in a[sym].items() for ub, y in b[sym].items() if x == y]
        what = [w for w, i in (("text", 0), ("descriptor", 1)) if {v[i] for v in va} != {v[i] for v in vb}]
        print(f"differs ({', '.join(what)}; A in {', '.join(a[sym])}; B in {', '.join(b[sym])}; equal: {', '.join(same) or 'none'}): {sym}")
    print(f"A: {len(a)} kernels in {sum(len(u) for u in a.values())} bodies; B: {len(b)} kernels in {sum(len(u) for u in b.values())} bodies; "
          f"{len(set(a) & set(b))} in both; {bad} difference(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
