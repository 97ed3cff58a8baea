#!/usr/bin/env python3
"""Compare the device assembly of two builds kernel by kernel: tools/asm_kernels_diff.py A.s B.s
(A.s / B.s: hipcc <Makefile flags> --cuda-device-only -S file.hip -o X.s)

A refactor of host code may change the ORDER in which templates are instantiated and with it the order of the functions in the
file and the function numbers inside local labels (.LBB12_3), but must not change any kernel. The files are cut into blocks at
every .section line and into the entries of the kernel metadata; function numbers in local labels, .file / .ident lines and the
per-translation-unit __hip_cuid symbol are normalised away; the two multisets of blocks must be equal and so must the sets of
kernel symbols. Exit status 0 = identical."""
import collections
import re
import sys


def blocks(path):
    out, cur, names, meta = [], [], set(), False
    for line in open(path):
        if re.match(r"\s*\.(file|ident)\b", line):
            continue
        line = re.sub(r"\.L(BB|func_begin|func_end|tmp|JTI|CPI|post_getpc)(\d+)", r".L\1N", line)
        line = re.sub(r"(Header|Parent Loop)( |=)BB\d+_", r"\1\2BBN_", line)  # (loop comments)
        line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", line)
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            names.add(m.group(1))
        if ".amdgpu_metadata" in line:
            meta = not meta
        if re.match(r"\s*\.section\b", line) or (meta and re.match(r"  - \.", line)):
            out.append("".join(cur))
            cur = []
        cur.append(line)
    out.append("".join(cur))
    return collections.Counter(out), names


def main():
    (a, na), (b, nb) = blocks(sys.argv[1]), blocks(sys.argv[2])
    only_a, only_b = a - b, b - a
    print(f"{len(na)} / {len(nb)} kernels; symbols only in A: {sorted(na - nb)}; only in B: {sorted(nb - na)}")
    print(f"{sum(a.values())} / {sum(b.values())} blocks; differing: {sum(only_a.values())} / {sum(only_b.values())}")
    for blk in list(only_a)[:3] + list(only_b)[:3]:
        print("----", blk[:400])
    return 0 if not only_a and not only_b and na == nb else 1


if __name__ == "__main__":
    sys.exit(main())
