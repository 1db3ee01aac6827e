"""-m gpu: no block of the device-memory pool is recycled while somebody still uses it.

All device memory of libsphx comes from the caching pool of csrc/sphx_common.hip, and DevBuf::release() is a bare pool_free: no
stream, no event.  Everything rests on one invariant -- a block returns to the pool only after every stream that was given it
has been waited for -- which is kept by a sync somewhere in every call that releases memory.  A suite that holds one object at
a time on one in-order stream, or syncs everything before it enables, disables, reads or closes, cannot notice a sync that is
missing; and a premature free gives no fault, only a few wrong doubles in somebody else's run.

So here objects live side by side (tests/live_worker.py, one child process per scene): the subject has N steps in flight --
prepare_steps(N), enqueue_steps(N), a pure replay -- when the risky call is made, on it or on a neighbour of the same sizes,
with capi.pool_poison_on_free(True, 3) filling every block with the word 3 the moment it is released.  The reference of every
object is the same sequence of calls on that object alone, with sync() in front of every risky call and the poison off;
everything an object returns must be the same bytes (tobytes()) in the scene as alone.  The quiescent observation of every kind
of object in a scene is checked against the oracle (pool_history_worker.check_fresh, the tolerances of test_gpu_resident.py /
test_gpu_mex_surface.py), so equal bytes cannot be equally wrong.

Not vacuous: the child reports the blocks poisoned and the pool hits of the neighbours' allocations, both of which must be
positive, and for every moment the host time from the return of enqueue_steps to the entry of the risky call, which must stay
below half of T_N, the time the subject's N steps take alone ("in flight for sure"; the child fails the scene as "not
exercised" otherwise).  profiles/r39_live_neighbours.txt has the measured run and two libraries broken on purpose.

The scenes: solo (every subject of pool_history_worker, poison off and on: one object in one stream order must not notice the
mode), samplers_in_flight (all nine samplers: enable with another configuration, reset, sample-now, draining read, disable),
reads_in_flight (download, monitor, pair list, prepare_steps with another count, advance by a chunk without a graph; 16 and 2
lanes), close_in_flight (a context, a batch closed with N steps in flight; a context, the stateless surface as the newcomer),
neighbour_churn (contexts, the stateless surface and a batch come and go beside a subject in flight), ring (an in-process
ring of two and of three slabs: a slab sampler's *_part_disable / *_part_enable on one slab, graph_prepare, the engines closed
one at a time in both orders; SPHX_SLAB_OVERLAP unset and `always`) and threads (three Python threads, each with an object
of its own).

Each child runs under the time limit of test_gpu_switches.py.  After a child that ended by a signal, an abort or its time limit
no further child is started: that end is to be diagnosed from what the child printed, not run again."""
import json
import os
import subprocess
import sys

import pytest

from test_gpu_switches import CHILD_SECONDS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "live_worker.py")
_abnormal = []  # what ended abnormally, if anything did

SOLO = ("ctx16", "ctx32", "ctx2", "ctx4dyn", "ctxK1", "ctx2tiles", "dual", "samplers", "batch4", "ring2", "surface")
# (scene, extra arguments of the child, environment of the child)
CHILDREN = [pytest.param("solo", ["--subjects", s], dict(SPHX_DEBUG_SWITCHES="tiles_be_from_1" if s == "ctx2tiles" else ""), id=f"solo-{s}")
            for s in SOLO]
CHILDREN += [pytest.param(s, [], {}, id=s) for s in ("samplers_in_flight", "reads_in_flight", "close_in_flight", "neighbour_churn")]
CHILDREN += [pytest.param("ring", [], dict(SPHX_SLAB_OVERLAP=None), id="ring"),
             pytest.param("ring", [], dict(SPHX_SLAB_OVERLAP="always"), id="ring-overlap"),
             pytest.param("threads", [], {}, id="threads")]


def run_child(scene, extra, env_more):
    env = dict(os.environ, SPHX_DEBUG_SWITCHES="")
    for k, v in env_more.items():
        if v is None:
            env.pop(k, None)
        else:
            env[k] = v
    cmd = [sys.executable, WORKER, "--scene", scene] + list(extra)
    try:
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_SECONDS)
    except subprocess.TimeoutExpired as e:
        _abnormal.append(f"{scene}: time limit of {CHILD_SECONDS} s")
        pytest.fail(f"{_abnormal[0]}\n{(e.stdout or b'')[-3000:]}\n{(e.stderr or b'')[-3000:]}")
    if r.returncode != 0:
        _abnormal.append(f"{scene}: exit code {r.returncode}")  # (the child exits with 0 whenever it ran to the end)
        pytest.fail(f"{scene}: exit code {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("scene, extra, env_more", CHILDREN)
def test_no_block_is_recycled_while_in_use(scene, extra, env_more):
    if _abnormal:
        pytest.fail(f"not started: an earlier child ended abnormally ({_abnormal[0]})")
    out = run_child(scene, extra, env_more)
    assert out["scene"] == scene
    print(f"[live neighbours] {scene} {' '.join(extra)}: N {out['n_flight']}, T_N {out['t_n']} s, largest host time to a risky call "
          f"{out['gap_max']} s ({out['gap_worst']}), {out['moments']} moments, poisoned {out['poison']}, neighbours' pool "
          f"{out['neighbour_pool']}, pool {out['pool']}, {out['compared']} arrays compared, fresh {out['fresh']}, "
          f"{out['seconds']} s")
    # not vacuous: blocks were poisoned, and the neighbours' allocations were served from the cache
    assert out["poison"]["filled"] > 0, out["poison"]
    assert out["neighbour_pool"]["hits"] > 0, out["neighbour_pool"]
    assert out["moments"] > 0 and out["compared"] >= 20, (out["moments"], out["compared"])
    assert not out["threads_alive"], out["threads_alive"]
    # every quiescent kind of object against its oracle
    assert out["fresh"] and all(f["failures"] == 0 and f["arrays"] > 0 for f in out["fresh"]), out["fresh"]
    # the same bytes side by side as alone, every moment in flight for sure
    assert not out["differing"], f"{len(out['differing'])} outputs differ from the object's quiescent run:\n" + "\n".join(out["differing"][:30])
    assert not out["failures"], "\n".join(out["failures"][:30])
