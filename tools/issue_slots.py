#!/usr/bin/env python3
"""What a wave of a kernel issues, counted in `hipcc -S --cuda-device-only` output (no GPU needed):

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -mllvm -amdgpu-kernarg-preload-count=14 -S -o /tmp/resident.s \
        sph-poiseuille-flow_amd/csrc/sphx_resident.hip
    python3 tools/issue_slots.py /tmp/resident.s 'k_forcesILi16ELi320E' [more patterns]      # one listing: the blocks of each kernel
    python3 tools/issue_slots.py /tmp/before.s /tmp/after.s 'k_forcesILi16ELi320E' [...]      # two listings: the difference

Every instruction takes an issue slot of its wave (a lone wave issues one per four cycles, scalar ones included), so the counts
are static issue slots.  Per basic block (the entry and every .LBB label) and per kernel:

    VALU    vector-ALU instructions (v_...)          FP64   those of them on doubles (..._f64)      v_mov  those of them that only move
    SALU    scalar instructions other than loads and branches (waits and no-ops included)           saveexec  those that save the exec mask
    MEM     loads, stores and atomics of any kind (vector, LDS, scalar loads)                      BR     branches

With two listings the blocks are not matched (their numbering moves with every change): the totals of both, their difference,
and the FP64 instructions by opcode where the two differ -- a change that takes slots out must leave that multiset alone.
Counts are static: a block's weight on a wave's path is for the reader (tools/load_chain.py prints the loops)."""
import collections
import re
import subprocess
import sys

CLASSES = ("VALU", "FP64", "v_mov", "SALU", "saveexec", "MEM", "BR")
MEMORY = ("global_", "flat_", "buffer_", "scratch_", "ds_", "s_load_", "s_buffer_load_")


def classes(op):
    """The classes one instruction counts in."""
    if op.startswith(MEMORY):
        return ("MEM",)
    if op.startswith(("s_cbranch", "s_branch")):
        return ("BR",)
    if op.startswith("v_"):
        return ("VALU",) + (("FP64",) if "_f64" in op else ()) + (("v_mov",) if op.startswith("v_mov") else ())
    if op.startswith("s_"):
        return ("SALU",) + (("saveexec",) if "saveexec" in op else ())
    return ()


def kernels(path, pats):
    """{mangled name: [(block label, Counter of classes, Counter of FP64 opcodes)]} of the kernels whose name holds a pattern."""
    lines = open(path).read().split("\n")
    out = {}
    for k, l in enumerate(lines):
        m = re.match(r"^(_Z\S*):", l)
        if not m or not any(p in m.group(1) for p in pats):
            continue
        blocks = [("entry", collections.Counter(), collections.Counter())]
        for ln in lines[k + 1:]:
            if ln.startswith(".Lfunc_end"):
                break
            b = re.match(r"^(\.LBB\d+_\d+):", ln)
            if b:
                blocks.append((b.group(1), collections.Counter(), collections.Counter()))
                continue
            i = re.match(r"^\t([a-z_0-9]+)", ln)
            if i and not i.group(1).startswith("."):
                cl = classes(i.group(1))
                blocks[-1][1].update(cl)
                if "FP64" in cl:  # (by operation: the encoding the assembler was asked for is no part of it)
                    blocks[-1][2][re.sub(r"_(e32|e64|dpp|sdwa)$", "", i.group(1))] += 1
        out[m.group(1)] = blocks
    return out


def total(blocks):
    t, f = collections.Counter(), collections.Counter()
    for _, c, fp in blocks:
        t.update(c)
        f.update(fp)
    return t, f


def demangle(name):
    return subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0] or name


def row(label, c):
    return "%-16s" % label + " ".join("%s %4d" % (k, c[k]) for k in CLASSES) + "   slots %5d" % (c["VALU"] + c["SALU"] + c["MEM"] + c["BR"])


def main():
    paths = [a for a in sys.argv[1:] if a.endswith(".s")]
    pats = [a for a in sys.argv[1:] if not a.endswith(".s")]
    if len(paths) not in (1, 2) or not pats:
        sys.exit(__doc__)
    if len(paths) == 1:
        for name, blocks in kernels(paths[0], pats).items():
            print("== %s   (%d blocks)" % (demangle(name), len(blocks)))
            for label, c, _ in blocks:
                print("   " + row(label, c))
            print("   " + row("total", total(blocks)[0]))
            print()
        return 0
    a, b = kernels(paths[0], pats), kernels(paths[1], pats)
    for name in sorted(set(a) | set(b), key=demangle):
        print("== %s" % demangle(name))
        if name not in a or name not in b:
            print("   only in %s" % (paths[0] if name in a else paths[1]))
            continue
        (ta, fa), (tb, fb) = total(a[name]), total(b[name])
        d = collections.Counter({k: tb[k] - ta[k] for k in CLASSES})
        d["slots"] = 0
        print("   " + row("before", ta) + "   blocks %3d" % len(a[name]))
        print("   " + row("after", tb) + "   blocks %3d" % len(b[name]))
        print("   %-16s" % "difference" + " ".join("%s %+4d" % (k, d[k]) for k in CLASSES)
              + "   slots %+5d" % sum(d[k] for k in ("VALU", "SALU", "MEM", "BR")))
        ops = sorted(k for k in set(fa) | set(fb) if fa[k] != fb[k])
        print("   FP64 by opcode: " + ("the same multiset" if not ops else ", ".join("%s %d -> %d" % (k, fa[k], fb[k]) for k in ops)))
        print()
    return 0


if __name__ == "__main__":
    sys.exit(main())
