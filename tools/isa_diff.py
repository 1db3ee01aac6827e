#!/usr/bin/env python3
"""Which kernels differ between two device-only assembly listings of one translation unit (no GPU needed):
    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -o a.s sph-poiseuille-flow_amd/csrc/sphx_resident.hip
    tools/isa_diff.py a.s b.s
Compared per mangled name: the text from the function label to its .Lfunc_end plus the .amdhsa_kernel block, comments
dropped and basic-block labels (.LBB<n>_) renumbered.  Exit status 1 when anything was added, removed or changed."""
import re
import sys


def kernels(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", txt, re.S | re.M):
        name = m.group(1)
        body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), txt, re.S | re.M).group(0)
        text = re.sub(r"\.L(BB|func_end)\d+", r".L\1", body + m.group(2))
        lines = (re.sub(r"\s*;.*", "", ln).strip() for ln in text.split("\n"))
        out[name] = "\n".join(ln for ln in lines if ln)
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
added, removed = sorted(set(b) - set(a)), sorted(set(a) - set(b))
changed = sorted(k for k in set(a) & set(b) if a[k] != b[k])
for tag, names in (("added", added), ("removed", removed), ("changed", changed)):
    for k in names:
        print(tag, k)
print(f"{len(a)} kernels before, {len(b)} after: {len(added)} added, {len(removed)} removed, {len(changed)} changed")
sys.exit(1 if added or removed or changed else 0)
