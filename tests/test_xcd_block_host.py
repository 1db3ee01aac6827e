"""No GPU: the workgroup -> block mapping of a pass (csrc/sphx_xcd_block.hpp), compiled into a host program.

A pass whose workgroups are the physical blocks first + j, j in [0, nb), gives the k-th workgroup of physical residue
c = (first + j) & 7 the block c * per + k (per = nb >> 3) and the nb - 8 * per workgroups left over the blocks behind the eight
eighths.  For every nb in 1 ... 8 192 and first in {0, nb, 8 * ceil(nb / 8)} the program checks that
  - the mapping is a bijection onto [0, nb),
  - a block c * per + k, k < per, is always produced by a physical block of residue c,
  - it equals the statement with j0 = (c - first) & 7 and k = (j - j0) >> 3 written out, and
  - for first % 8 == 0 it equals the mapping of a pass that starts at block 0 as it was before (b < 8 per ? (b & 7) per + (b >> 3) : b)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sph-poiseuille-flow_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "sphx_xcd_block.hpp"

static int old_xcd_block(int b, int nb)
{
    const int per = nb >> 3;
    return b < (per << 3) ? (b & 7) * per + (b >> 3) : b;
}
static int stated(int first, int j, int nb)
{
    const int per = nb >> 3, c = (first + j) & 7, j0 = (c - first) & 7, k = (j - j0) >> 3;
    return k < per ? c * per + k : 8 * per + j0;
}

int main()
{
    long checked = 0;
    std::vector<int> hits;
    for (int nb = 1; nb <= 8192; ++nb) {
        const int per = nb >> 3;
        const int firsts[3] = {0, nb, 8 * ((nb + 7) / 8)};
        for (int first : firsts) {
            hits.assign(nb, 0);
            for (int j = 0; j < nb; ++j) {
                const int blk = sphx::xcd_block(first, j, nb);
                if (blk < 0 || blk >= nb) { printf("nb %d first %d j %d: block %d outside [0, nb)\n", nb, first, j, blk); return 1; }
                if (++hits[blk] > 1) { printf("nb %d first %d j %d: block %d taken twice\n", nb, first, j, blk); return 1; }
                if (blk < 8 * per && blk / per != ((first + j) & 7)) {
                    printf("nb %d first %d j %d: block %d of eighth %d from residue %d\n", nb, first, j, blk, blk / per, (first + j) & 7);
                    return 1;
                }
                if (blk != stated(first, j, nb)) { printf("nb %d first %d j %d: %d, stated %d\n", nb, first, j, blk, stated(first, j, nb)); return 1; }
                if (first % 8 == 0 && blk != old_xcd_block(j, nb)) {
                    printf("nb %d first %d j %d: %d, before %d\n", nb, first, j, blk, old_xcd_block(j, nb));
                    return 1;
                }
                ++checked;
            }
        }
    }
    printf("ok %ld\n", checked);
    return 0;
}
"""


def _compiler():
    for cand in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = cand and shutil.which(cand)
        if path:
            return path
    pytest.fail("no C++ compiler found (g++, c++ or clang++)")


def test_xcd_block_is_a_bijection_that_keeps_an_eighth_on_its_residue(tmp_path):
    src, exe = tmp_path / "xcd_block_host.cpp", tmp_path / "xcd_block_host"
    src.write_text(PROGRAM)
    subprocess.run([_compiler(), "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # every (nb, first, j): 3 * sum(nb) evaluations
    assert r.stdout.split() == ["ok", str(3 * 8192 * 8193 // 2)], r.stdout[-2000:]
