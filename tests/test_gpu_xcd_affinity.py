"""-m gpu: which workgroup takes which block of a pass changes no result.

The A half of the fused E|A launch starts at physical block nb of its grid and numbers its blocks by the physical residue of
its workgroups (xcd_block, csrc/sphx_xcd_block.hpp), so that an eighth of the particle range meets the same XCD in every pass
of a step; SPHX_DEBUG_SWITCHES=no_xcd_align numbers it as if it started at block 0, as it was before.  Both are bijections of
the same blocks and no sum changes its order: the nine fields, t, dt and the step count must be equal bit for bit after 20
steps with a re-binning every 8th, and both must launch the same kernels the same number of times from as many graphs.  The
library reads the switches once per process, so each variant runs tests/xcd_affinity_worker.py as a fresh child under its own
time limit; after a child that ends by a signal, an abort or its time limit no further child is started.

Cases (xcd_affinity_worker.CASES): 300 workgroups at 16 lanes per particle (the headline's shape, the A half starts at residue
4), 235 at 32 lanes, 320 at 16 lanes (residue 0: the two numberings are one mapping), 625 at 8 lanes (the large-channel form of
the fused launch), and a batch of three members of the 235-workgroup channel.  The batch forms of the kernels number their
blocks as before under either setting (profiles/r27_xcd_affinity.txt section 5): that case holds the switch to leaving a batch
alone, and member 0 to the standalone channel bit for bit.  Every test asserts from kernel_forms / schedule that the fused
launch was in fact used."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "xcd_affinity_worker.py")
CHILD_SECONDS = 120
_abnormal = []  # what ended abnormally, if anything did

NAMES = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B", "t", "dt_last", "vmax", "step")
# case -> (workgroups of a pass, compact kernels?, members)
CASES = {"nb300": (300, True, 1), "nb235": (235, True, 1), "nb320": (320, True, 1), "nb625w": (625, False, 1),
         "batch3": (235, True, 3)}


def _child(case, switches, dump):
    if _abnormal:
        pytest.fail(f"not started: an earlier child ended abnormally ({_abnormal[0]})")
    env = dict(os.environ, SPHX_DEBUG_SWITCHES=switches)
    cmd = [sys.executable, WORKER, "--case", case, "--dump", str(dump)]
    try:
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_SECONDS)
    except subprocess.TimeoutExpired as e:
        _abnormal.append(f"{case} [{switches}]: time limit of {CHILD_SECONDS} s")
        pytest.fail(f"{_abnormal[0]}\n{(e.stdout or b'')[-3000:]}\n{(e.stderr or b'')[-3000:]}")
    if r.returncode != 0:
        _abnormal.append(f"{case} [{switches}]: exit code {r.returncode}")
        pytest.fail(f"{_abnormal[0]}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(lines[0])
    assert out["switches"] == switches and out["case"] == case
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_numbering_changes_no_bit(case, tmp_path):
    blocks, compact, members = CASES[case]
    runs = {sw: _child(case, sw, tmp_path / (sw or "default")) for sw in ("", "no_xcd_align")}
    for sw, out in runs.items():
        assert out["blocks"] == blocks, out
        assert out["forms"]["walk_kernels"] == (not compact), out["forms"]
        assert (out["schedule"]["fuse_ea"], out["schedule"]["tail_clock"], out["schedule"]["dynamic"]) == (1, 1, 0), out["schedule"]
        assert out["steps"] == 20 and out["rebins"] >= 1, out  # 20 steps, re-binning every 8th: at least one is crossed
        assert out["graph_stats"]["slots_replayed"] > 0, out["graph_stats"]
        assert out["launches"].get("k_continuity_density", 0) >= 6, out["launches"]  # 9 traced steps, one of them re-bins
        if members > 1:
            assert out["batch_info"]["n_members"] == members and out["batch_steps"] == [20] * members, out
            assert out["batch_graph_stats"]["slots_replayed"] > 0, out["batch_graph_stats"]
    a, b = runs[""], runs["no_xcd_align"]
    print(f"[xcd] {case}: {blocks} workgroups, re-binnings {a['rebins']}, launches {a['launches']}")
    assert a["rebins"] == b["rebins"], (a["rebins"], b["rebins"])
    # the same kernels, the same number of times, replayed from as many graphs
    assert a["launches"] == b["launches"], (a["launches"], b["launches"])
    assert a["graph_stats"] == b["graph_stats"], (a["graph_stats"], b["graph_stats"])
    prefixes = [""] + ([f"m{m}_" for m in range(members)] if members > 1 else [])
    differs = []
    for prefix in prefixes:
        for name in NAMES:
            x = np.load(tmp_path / "default" / f"{prefix}{name}.npy")
            y = np.load(tmp_path / "no_xcd_align" / f"{prefix}{name}.npy")
            assert x.size > 0 and x.shape == y.shape and x.dtype == y.dtype, (prefix, name)
            if x.tobytes() != y.tobytes():
                differs.append(prefix + name)
    assert not differs, differs
    if members > 1:  # member 0 of the batch is the standalone channel, bit for bit
        for name in NAMES:
            x, y = np.load(tmp_path / "default" / f"{name}.npy"), np.load(tmp_path / "default" / f"m0_{name}.npy")
            assert x.tobytes() == y.tobytes(), name
