#!/usr/bin/env python3
"""The chain of memory requests and waits of one kernel in `hipcc -S --cuda-device-only` output (no GPU needed):

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -o /tmp/resident.s sph-poiseuille-flow_amd/csrc/sphx_resident.hip
    python3 tools/load_chain.py /tmp/resident.s 'k_kgcILi16E' ['k_forcesILi16E' ...]

Prints, in program order, the scalar loads, the vector loads, the wait instructions and the loop headers (labels that a
later branch jumps back to) of every kernel whose mangled name contains a pattern -- nothing else.  Runs of loads are folded
into one line each ("s_load x5: dwordx2 dwordx4 ..."), so that a request wave reads as one line and every line between two
waits is one link of the chain.  A summary counts the waits in front of the first DEPENDENT request: the first vector load
issued behind a wait for vector loads, so one whose address may come out of memory (the first neighbour gather of a pass).
A kernel built for kernel-argument preload starts with a prologue that loads its leading arguments itself and branches to the
256-byte-aligned entry a wave with preloaded arguments starts at: the listing marks that entry, and the summary counts from it."""
import re
import subprocess
import sys

SCALAR = ("s_load_", "s_buffer_load_")


def kind(op):
    if op.startswith(SCALAR):
        return "s_load"
    if op.startswith(("global_load_", "flat_load_", "buffer_load_", "scratch_load_")):
        return "v_load"
    if op.startswith(("ds_read", "ds_load")):
        return "lds_read"
    if op.startswith("s_waitcnt"):
        return "wait"
    return None


def width(op):
    return re.sub(r"^(s_buffer_load_|s_load_|global_load_|flat_load_|buffer_load_|scratch_load_|ds_read_?|ds_load_?)", "", op)


def chain(lines, start, end):
    body, labels = [], {}
    for k in range(start, end):
        m = re.match(r"^(\.LBB\d+_\d+):", lines[k])
        if m:
            labels[m.group(1)] = len(body)
            body.append((k + 1, "label", m.group(1)))
            continue
        if re.match(r"^\t\.p2align\s+8", lines[k]) and body and body[-1][1] == "s_branch":
            # a kernel built for kernel-argument preload: what stood above is the prologue that loads the leading arguments
            # itself (firmware without preload enters there); a wave that got them in registers enters HERE, 256 bytes on
            body.append((k + 1, "entry", ""))
            continue
        m = re.match(r"^\t([a-z_0-9]+)\s*([^;]*)", lines[k])
        if m and not m.group(1).startswith("."):
            body.append((k + 1, m.group(1), m.group(2).strip()))
    loops = {}  # header label -> line of the last backward branch to it
    for idx, (ln, op, args) in enumerate(body):
        if op.startswith(("s_cbranch", "s_branch")):
            tgt = args.split()[-1] if args else ""
            if tgt in labels and labels[tgt] <= idx:
                loops[tgt] = ln
    out, run = [], None  # run = [kind, first line, [widths]]

    def flush():
        nonlocal run
        if run:
            out.append((run[1], "%-8s x%-2d %s" % (run[0], len(run[2]), " ".join(run[2]))))
            run = None

    waits_s, waits_v, first_gather = 0, 0, None
    for ln, op, args in body:
        if op == "entry":
            flush()
            out.append((ln, "---- entry with preloaded arguments (the lines above: the fallback prologue, not run then) ----"))
            waits_s, waits_v, first_gather = 0, 0, None  # the summary counts the preloaded path
            continue
        if op == "label":
            if args in loops:
                flush()
                out.append((ln, "loop %s {   (back edge at line %d)" % (args, loops[args])))
            continue
        k = kind(op)
        if k is None:
            continue
        if k == "wait":
            flush()
            out.append((ln, "%s %s" % (op, args)))
            if first_gather is None:
                if "lgkmcnt" in args:
                    waits_s += 1
                if "vmcnt" in args:
                    waits_v += 1
            continue
        if k == "v_load" and waits_v and first_gather is None:
            first_gather = ln
        if run and run[0] == k:
            run[2].append(width(op))
        else:
            flush()
            run = [k, ln, [width(op)]]
    flush()
    return out, waits_s, waits_v, first_gather


def main():
    path, pats = sys.argv[1], sys.argv[2:]
    lines = open(path).read().split("\n")
    for pat in pats:
        hits = [k for k, l in enumerate(lines) if re.match(r"^_Z\S*" + re.escape(pat) + r"\S*:", l)]
        if not hits:
            print("== %s: no such kernel" % pat)
            continue
        for start in hits:
            name = lines[start].split(":")[0]
            end = next(k for k in range(start, len(lines)) if lines[k].startswith(".Lfunc_end"))
            dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0]
            out, ws, wv, fg = chain(lines, start, end)
            print("== %s   (lines %d-%d)" % (dem or name, start + 1, end))
            for ln, text in out:
                print("%7d  %s" % (ln, text))
            print("   -- waits in front of the first dependent vector load (line %s): %d with lgkmcnt, %d with vmcnt"
                  % (fg, ws, wv))
            print()


if __name__ == "__main__":
    main()
