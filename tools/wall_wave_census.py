#!/usr/bin/env python3
"""Which waves of the compact passes hold a wall row, counted on the CPU from bench.py's own start (no GPU needed):

    python3 tools/wall_wave_census.py C2 16 320 256        # workload, lanes per particle, workgroup sizes

The state is geometry.developed_state(jitter 0.05, seed 12345); the fluid is ordered by cell (columns and rows of 2h + skin, the
skin of the static schedule at K = 16: 2 * 15 * 0.035 h), then by index, as the device bins it; a wave holds 64 / lanes
consecutive particles, a workgroup threads / lanes.  A particle has a wall row when a wall particle lies within 2h of it (the
minimum image in x).  Prints the share of particles, waves and workgroups without one (profiles/r49_wall_rows.txt)."""
import importlib
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    wl, lanes, sizes = sys.argv[1], int(sys.argv[2]), [int(a) for a in sys.argv[3:]] or [256]
    cfg, geo = importlib.import_module(bench.PKG + ".config"), importlib.import_module(bench.PKG + ".geometry")
    name, kw = bench.parse_workload(wl)
    prm = cfg.params_from_values(end_time=1e9, **kw)
    parts = geo.init_particles(prm)
    pos, _ = geo.developed_state(prm, parts, jitter=0.05, seed=12345)
    nf = parts["n_fluid"]
    f, w = pos[:nf], pos[nf:]
    near = np.zeros(nf, dtype=bool)
    for lo in range(0, nf, 2048):
        dx = f[lo:lo + 2048, None, 0] - w[None, :, 0]
        dx -= prm.DL * np.round(dx / prm.DL)
        dy = f[lo:lo + 2048, None, 1] - w[None, :, 1]
        near[lo:lo + 2048] = np.any(dx * dx + dy * dy < (2.0 * prm.h) ** 2, axis=1)
    cs = 2.0 * prm.h + 2.0 * 15 * 0.035 * prm.h
    ncx = max(1, math.floor(prm.DL / cs))
    y0 = float(pos[:, 1].min())
    ncy = math.ceil((float(pos[:, 1].max()) - y0 + 1e-12) / cs) + 1
    cx = np.clip(np.floor(f[:, 0] * (ncx / prm.DL)).astype(np.int64), 0, ncx - 1)
    cy = np.clip(np.floor((f[:, 1] - y0) / cs).astype(np.int64), 0, ncy - 1)
    order = np.lexsort((np.arange(nf), cx * ncy + cy))

    def groups(per):
        n = -(-nf // per)
        has = np.zeros(n * per, dtype=bool)
        has[:nf] = near[order]
        return n, int(np.count_nonzero(has.reshape(n, per).any(axis=1)))

    n_w, wall_w = groups(64 // lanes)
    print(f"{name}: {nf} fluid, {len(w)} wall particles, {ncx} x {ncy} cells, {lanes} lanes per particle")
    print(f"  particles with a wall neighbour {np.count_nonzero(near)} ({100.0 * np.count_nonzero(near) / nf:.1f} %)")
    print(f"  waves {n_w}, with a wall row {wall_w} ({100.0 * wall_w / n_w:.1f} %)")
    for blk in sizes:
        n_g, wall_g = groups(blk // lanes)
        print(f"  workgroups of {blk} threads {n_g}, wall-free {n_g - wall_g} ({100.0 * (n_g - wall_g) / n_g:.1f} %)")


if __name__ == "__main__":
    main()
