"""-m gpu: what an object computes must not depend on what the device-memory pool held before.

All device memory of libsphx comes from the caching pool of csrc/sphx_common.hip, which hands a freed block to the next request
of its size class as it was returned: DevBuf::alloc clears nothing.  ctx_alloc zeroes about half of a context's arrays; the
stateless modes of csrc/sphx_pairlist.hip take every output and every temporary from the pool on each call.  Results are right
only if some kernel writes every row before it is read or returned -- wall rows, rows without a pair, list entries beyond the
count, lanes beyond n in the padded stride, the lazily written outputs of the walk kernels, rows a re-binning does not touch.

A suite that runs in one process on a handful of shapes cannot see a violation: a row read before it is written usually holds
what the previous test of the same shape left in the same size class, very often the right answer.  So every subject here runs
in a child process of its own (tests/pool_history_worker.py) four times over -- as the first device work of the process, after
a foreign predecessor of the same sizes that leaves valid but wrong data behind, after capi.pool_scrub(3) has filled every
cached free block with the word 3, and after a predecessor that ran into NaN -- and everything it returns (downloads, monitors,
pair lists, status, counters, every sampler's output) must be the same bytes all four times.  The library promises bit-identical
results between runs (csrc/sphx_pairlist.hip, header), so this is byte equality (tobytes(): NaN equals NaN, -0.0 differs from
0.0); no tolerance is involved.  The scrub word is small on purpose: an int read before it is written stays an in-bounds
index, count or cell on these shapes, so the poison itself cannot make a kernel fault; as a double the word pair is a
denormal, invisible inside a sum and visible bit for bit in a returned row that nobody wrote.

Not vacuous: capi.pool_stats() around every subject shows that in the three later runs no allocation went to hipMalloc
(`misses` unchanged) -- every block the subject took had a previous owner -- and the scrub reports the blocks it filled.
Not four equal wrong answers: the child checks the fresh run against the oracle at the tolerances of test_gpu_resident.py
(rtol 1e-9, atol_scale 1e-10; tau 1e-8 / 1e-9), the step-0 state against the input and the step-0 pair count against
oracle.neighbor_search, a ring against a single context as tests/test_slab.py does, the stateless surface against
helpers.oracle_surface mode by mode at test_gpu_mex_surface.py's tolerances, the dual-rate loop against
tests/dual_rate_reference.py, and one sample of the field map and of the probes against profile.shepard_field /
shepard_points at the sampler tests' 1e-12.

The subjects (tests/pool_history_worker.py, SUBJECTS): contexts on the compact kernels at 16 and 32 lanes, on the walk kernels
at 2 lanes, with the device-decided re-binning at 4 lanes, re-binning every step, the tile forms and coded lists under
tiles_be_from_1, the dual-rate loop, the four samplers; a batch of four members with the samplers on; an in-process ring of two
slabs with its samplers, with the default cadence and rebuild_every = 5; the stateless surface on the search's own list and on
lists with skipped, repeated and empty rows.  Each is read before the first step (state, pair count and pair list: rho, p,
force, Vol, B and the wall shear exist only after a step), after 1 step and after 35.  The probes sit on x = 0, mid-channel,
within 2h of the bottom wall and on the top wall line beyond x = DL; a void probe cannot be had on this state, since
probes_enable refuses a point outside [0, DH] and the channel has no void (tests/test_gpu_probes.py::test_void_is_no_value
covers one).  profiles/r26_pool_history.txt has the measured run and two broken libraries the test tells from the right one.

Each child runs under the time limit of test_gpu_switches.py.  After a child that ended by a signal, an abort or its time limit
no further child is started: that end is to be diagnosed from what the child printed, not run again."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_switches import CHILD_SECONDS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "pool_history_worker.py")
HISTORIES = ("fresh", "foreign", "scrub3", "nan")
_abnormal = []  # what ended abnormally, if anything did

WALK = dict(walk_kernels=True, lds_tiles=True, tiles_abe=False, coded_lists=False)
COMPACT = dict(walk_kernels=False, lds_tiles=False, tiles_abe=False, coded_lists=False)
# subject -> (SPHX_DEBUG_SWITCHES of the child, the kernel forms the context must have chosen or None, lanes per particle)
SUBJECTS = {
    "ctx16": ("", COMPACT, 16),
    "ctx32": ("", COMPACT, 32),
    "ctx2": ("", WALK, 2),
    "ctx4dyn": ("", None, 4),
    "ctxK1": ("", COMPACT, 16),
    "ctx2tiles": ("tiles_be_from_1", dict(WALK, tiles_abe=True, coded_lists=True), 2),
    "dual": ("", COMPACT, None),
    "samplers": ("", COMPACT, 16),
    "batch4": ("", None, None),
    "ring2": ("", None, None),
    "surface": ("", None, None),
}


def first_difference(name, a, b):
    """Where two arrays of one name differ, byte for byte: the first rows."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"{name}: {a.dtype}{a.shape} against {b.dtype}{b.shape}"
    x = np.ascontiguousarray(a).reshape(-1).view(np.uint8).reshape(a.size, -1) if a.size else np.zeros((0, 1), np.uint8)
    y = np.ascontiguousarray(b).reshape(-1).view(np.uint8).reshape(b.size, -1) if b.size else np.zeros((0, 1), np.uint8)
    flat = np.flatnonzero(np.any(x != y, axis=1))
    where = [tuple(int(v) for v in np.unravel_index(f, a.shape)) if a.ndim else () for f in flat[:4]]
    shown = ", ".join(f"{w}: {a[w].item()!r} against {b[w].item()!r}" for w in where)
    return f"{name}: {len(flat)} of {a.size} elements differ, first at {shown}"


def compare_histories(dump):
    """Every dumped array of every later history against the fresh run's: the same names, the same bytes."""
    runs = {}
    for h in HISTORIES:
        with np.load(os.path.join(dump, h + ".npz")) as z:
            runs[h] = {k: z[k] for k in z.files}
    fresh = runs["fresh"]
    assert len(fresh) >= 20, sorted(fresh)
    problems = []
    for h in HISTORIES[1:]:
        if set(runs[h]) != set(fresh):
            problems.append(f"fresh / {h}: different outputs {sorted(set(runs[h]) ^ set(fresh))[:6]}")
        for k in sorted(set(runs[h]) & set(fresh)):
            if fresh[k].tobytes() != runs[h][k].tobytes() or fresh[k].shape != runs[h][k].shape:
                problems.append(f"fresh / {h}: " + first_difference(k, fresh[k], runs[h][k]))
    return len(fresh), problems


@pytest.mark.parametrize("subject", list(SUBJECTS))
def test_results_do_not_depend_on_recycled_memory(subject, tmp_path):
    if _abnormal:
        pytest.fail(f"not started: an earlier child ended abnormally ({_abnormal[0]})")
    switches, forms, lanes = SUBJECTS[subject]
    env = dict(os.environ, SPHX_DEBUG_SWITCHES=switches)
    dump = str(tmp_path / subject)
    cmd = [sys.executable, WORKER, "--subject", subject, "--dump", dump]
    try:
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_SECONDS)
    except subprocess.TimeoutExpired as e:
        _abnormal.append(f"{subject}: time limit of {CHILD_SECONDS} s")
        pytest.fail(f"{_abnormal[0]}\n{(e.stdout or b'')[-3000:]}\n{(e.stderr or b'')[-3000:]}")
    if r.returncode != 0:
        _abnormal.append(f"{subject}: exit code {r.returncode}")  # (the child exits with 0 whenever it ran to the end)
        pytest.fail(f"{subject}: exit code {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(lines[0])
    assert out["subject"] == subject and out["switches"] == switches
    print(f"[pool history] {subject}: {out['n_arrays']} arrays, seconds {out['seconds']}, pool {out['pool']}, scrubbed "
          f"{out['scrubbed']} blocks, hits / misses {out['deltas']}")
    # the subject is the one meant
    if forms is not None:
        assert out["facts"]["forms"] == forms, out["facts"]
    if lanes is not None:
        assert out["facts"]["tuning"]["lanes_per_particle"] == lanes, out["facts"]
    if subject == "dual":
        assert out["facts"]["substeps"] > 1, out["facts"]
    elif "substeps" in out["facts"]:
        assert out["facts"]["substeps"] == 1, out["facts"]
    # not vacuous: the scrub found blocks to fill, and every block of a later run was a recycled one
    assert out["scrubbed"] > 0, out
    for h in HISTORIES[1:]:
        assert out["deltas"][h]["misses"] == 0 and out["deltas"][h]["hits"] > 0, (h, out["deltas"])
    # the same bytes whatever the pool held
    n, problems = compare_histories(dump)
    assert n == out["n_arrays"]
    assert not problems, f"{len(problems)} outputs depend on what the pool held before:\n" + "\n".join(problems[:20])
    assert not any(out["differing"].values()), out["differing"]
    # and the right ones
    assert not out["failures"], out["failures"]
