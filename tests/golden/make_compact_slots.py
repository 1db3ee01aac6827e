#!/usr/bin/env python3
"""Record tests/golden/compact_slots_<case>_lpp<lanes>.npz (needs a GPU): what tests/compact_slots_worker.py writes, taken with the
library of the commit BEFORE the compact passes lost their issue slots.

    SPHX_LIB=/path/to/that/commit/libsphx.so python tests/golden/make_compact_slots.py

SPHX_LIB is required: a recording made with the library under test would pin nothing.  The worker runs once per block size
(block_256, block_320), each in a fresh child under its own time limit; the two must agree to the byte before anything is written,
and the schedule must be the one the test asks for.  After a child that ends abnormally nothing more is started."""
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
import compact_slots_worker as worker  # noqa: E402

ARRAYS = worker.FIELDS + worker.SCALARS


def child(blk, out_dir):
    env = dict(os.environ, SPHX_DEBUG_SWITCHES=f"block_{blk}")
    r = subprocess.run([sys.executable, os.path.join(TESTS, "compact_slots_worker.py"), out_dir], env=env, cwd=ROOT,
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
            for k in ARRAYS:
                assert a[k].tobytes() == b[k].tobytes(), (run, k)
            assert f["steps"] == worker.STEPS and f["finite"] and f["n_fluid"] == 483 and f["n_wall"] == 184 and f["n_cell_x"] == 5, f
            assert f["fuse_ea"] == 1 and f["tail_clock"] == 1 and f["rebins"] == facts[320][run]["rebins"], f
            assert f["rebins"] == 2 or (run.startswith("rest") and f["rebins"] >= 1), f  # (the test holds `rest` to the recorded count)
            assert facts[320][run]["block_size"] == 320 and f["block_size"] == 256
            np.savez_compressed(os.path.join(HERE, f"compact_slots_{run}.npz"), **{k: a[k] for k in ARRAYS},
                                rebins=np.asarray(f["rebins"]))
            print("wrote", f"compact_slots_{run}.npz")


if __name__ == "__main__":
    main()
