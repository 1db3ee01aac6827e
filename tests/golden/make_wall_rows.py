#!/usr/bin/env python3
"""Record tests/golden/wall_rows_<case>_lpp<lanes>.npz (needs a GPU): what tests/wall_rows_worker.py writes, taken with the
library of the commit BEFORE pass CD of the compact kernels kept the pairs of its prefetched wall rows.

    SPHX_LIB=/path/to/that/commit/libsphx.so python tests/golden/make_wall_rows.py

SPHX_LIB is required: a recording made with the library under test would pin nothing.  The worker runs once per block size
(block_256, block_320), each in a fresh child under its own time limit; the two must agree to the byte before anything is
written.  Beside the arrays a file holds the re-binnings of the run and the grid the device reported (cell columns and rows,
skin), which tests/test_wall_rows_cases.py takes its CPU census of wave classes on.  After a child that ends abnormally
nothing more is started."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
import wall_rows_worker as worker  # noqa: E402


def child(blk, out_dir):
    env = dict(os.environ, SPHX_DEBUG_SWITCHES=f"block_{blk}")
    r = subprocess.run([sys.executable, os.path.join(TESTS, "wall_rows_worker.py"), out_dir], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=240)
    if r.returncode != 0:
        sys.exit(f"block_{blk}: exit code {r.returncode}; nothing more is started\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["runs"]


def main():
    if not os.environ.get("SPHX_LIB"):
        sys.exit("set SPHX_LIB to the parent commit's libsphx.so")
    with tempfile.TemporaryDirectory() as tmp:
        dirs = {blk: os.path.join(tmp, f"block_{blk}") for blk in (256, 320)}
        facts = {blk: child(blk, d) for blk, d in dirs.items()}
        for run, f in facts[256].items():
            print(run, f, facts[320][run])
            a = np.load(os.path.join(dirs[256], run + ".npz"))
            b = np.load(os.path.join(dirs[320], run + ".npz"))
            for k in worker.ARRAYS:
                assert a[k].tobytes() == b[k].tobytes(), (run, k)
            assert f["finite"] and f["fuse_ea"] == 1 and f["tail_clock"] == 1 and f["rebins"] == facts[320][run]["rebins"], f
            assert f["block_size"] == 256 and facts[320][run]["block_size"] == (256 if run.startswith(worker.ALWAYS_256) else 320)
            if run.startswith("batch4"):
                assert f["members_equal_contexts"] and f["steps"] == [worker.STEPS] * worker.MEMBERS, f
            else:
                assert f["steps"] == worker.STEPS and f["substeps"] == (3 if run.startswith("dual_rate") else 1), f
            np.savez_compressed(os.path.join(HERE, f"wall_rows_{run}.npz"), **{k: a[k] for k in worker.ARRAYS},
                                rebins=np.asarray(f["rebins"]), n_cell_x=np.asarray(f["n_cell_x"]), n_cell_y=np.asarray(f["n_cell_y"]),
                                skin=np.asarray(f["skin"]))
            print("wrote", f"wall_rows_{run}.npz")


if __name__ == "__main__":
    main()
