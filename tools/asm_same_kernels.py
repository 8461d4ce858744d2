#!/usr/bin/env python3
"""Do two `make asm` outputs hold the same kernels, whatever order they were emitted in?

    python3 tools/asm_same_kernels.py parent/build/rt_render.s build/rt_render.s

A kernel's position in the file follows the order in which the host code first names its
instantiation, so moving a launch moves a kernel.  This splits both files into sections (one per
function or kernel descriptor) and the metadata into its per-kernel entries, replaces the function
ordinal in local labels (.LBB<n>_, .Lfunc_end<n>, ...) and compares the two sets.  Exit status 0:
every piece of one file is in the other, byte for byte."""
import re
import sys
from collections import Counter


def pieces(path):
    text = open(path).read()
    text = re.sub(r"(\.L|\b)(BB|func_begin|func_end|tmp|JTI)\d+", r"\1\2#", text)  # (.LBB52_3 and "Header=BB52_3")
    text = re.sub(r"^\s*\.(file|loc|ident)\b.*\n", "", text, flags=re.M)
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_#", text)  # (a hash of the source file)
    body, _, meta = text.partition("\t.amdgpu_metadata")
    out = Counter(re.split(r"(?m)^(?=\t\.section\t)", body))
    out.update(re.split(r"(?m)^(?=  - \.agpr_count)", meta))
    return out


a, b = pieces(sys.argv[1]), pieces(sys.argv[2])
only_a, only_b = a - b, b - a
for tag, d in (("only in " + sys.argv[1], only_a), ("only in " + sys.argv[2], only_b)):
    for p in d:
        print(f"{tag}: {p.strip().splitlines()[0][:120] if p.strip() else '(blank)'} ({len(p.splitlines())} lines)")
print(f"{sum(a.values())} pieces, {sum(only_a.values()) + sum(only_b.values())} differ")
sys.exit(1 if only_a or only_b else 0)
