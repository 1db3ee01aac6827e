"""-m gpu: the leading arguments of the compact step kernels at 16 and 32 lanes per particle (sphx_kernels.hpp, "Leading arguments").

k_kgc, k_forces, k_forces_hist, k_continuity_compact, k_continuity_rebin, k_continuity_density and k_density_walk take the clock,
the number of workgroups of the pass with its flag, the row counts, the list, its stride and some own-record pointers as plain
parameters in front of their structs, and write them over the structs' fields.  The host takes each value from the view it passes
by value (hot_* in sphx_resident.hip).  What can go wrong is a value that disagrees with its struct at one launch site, or in one
captured phase of the cycle (graphs are captured per parity, layout and position) -- a list of the other parity, a stride of the
other layout, a workgroup count that misses the tail.  So: every launch site against the oracle, the same steps cut into
different calls (other graphs, and no graph at all) to the bit, the packed flag of the dual-rate loop, and a batch -- whose "_b"
forms take no leading arguments -- against standalone contexts to the bit.

Channel: tests/test_gpu_load_chains.py's -- dp = 0.05, DL = 1.5, DH = 1: 600 fluid particles, seven cell columns (the re-binning
step is the folded one); 37.5 workgroups at 16 lanes per particle (a partial last workgroup, both branches of xcd_block), 75 at 32.
Start: geometry.developed_state, jitter 0.2 dp, seed 21.  Bound: tests/test_gpu_headline_parity.py's for these lengths,
RTOL[20] = 1e-10 in max|a - b| / max|b| per field (the sides differ in summation order only); the dual-rate case at
tests/test_gpu_dual_rate_parity.py's bound, the same figure, against tests/dual_rate_reference.py.
"""
import numpy as np
import pytest

import dual_rate_reference

pytestmark = pytest.mark.gpu

FIELDS = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B")
RTOL = 1e-10  # tests/test_gpu_headline_parity.py, RTOL[20]; tests/test_gpu_dual_rate_parity.py, RTOL
DP, DL = 0.05, 1.5
_REF = {}  # oracle runs by number of steps: computed once, never changed


def _start(cfgmod, geom, seed=21):
    prm = cfgmod.params_from_values(dp=DP, DL=DL)
    parts = dict(geom.init_particles(prm))
    pos, vel = geom.developed_state(prm, parts, jitter=0.2, seed=seed)
    assert parts["n_fluid"] == 600 and abs(prm.DH - 1.0) < 1e-12
    parts.update(pos=pos, vel=vel)
    return prm, parts


def _oracle(oracle, prm, parts, n_steps):
    if n_steps not in _REF:
        ref = oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=n_steps, enable_sort=False)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[n_steps] = ref
    return _REF[n_steps]


def _run(capi, prm, parts, calls, **kw):
    """calls: the step budgets of successive advance() calls -> last status, download, facts about the context"""
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        info = dict(tuning=ctx.tuning(), policy=ctx.grid_policy(), sched=ctx.schedule(), substeps=ctx.substeps())
        for n in calls:
            st = ctx.advance(1e9, max_steps=n)
        got = ctx.download()
        info["sched_after"] = ctx.schedule()
    return st, got, info


def _errors(got, ref):
    out = {}
    for k in FIELDS:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape and np.all(np.isfinite(a)), k
        out[k] = float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))
    return out


def _same(name, a, b):
    (sa, ga), (sb, gb) = a, b
    assert sa == sb, (name, sa, sb)
    for k, v in ga.items():
        assert np.array_equal(v, gb[k]), f"{name}: {k} differs"


# 20 steps of the default schedule cross the scheduled re-binning of step 16 (k_forces_hist, k_continuity_rebin, then the cell
# sweep and the first fused launch of the new cycle); rebuild_every = 1: no list is walked, every pass is launched on its own;
# rebuild_every = 3: four short cycles, the fused launch entered from every parity and layout
@pytest.mark.parametrize("lanes", [16, 32])
@pytest.mark.parametrize("n_steps,rebuild_every", [(20, 0), (6, 1), (12, 3)])
def test_every_launch_site_against_the_oracle(n_steps, rebuild_every, lanes, cfgmod, geom, capi, oracle, capsys):
    prm, parts = _start(cfgmod, geom)
    kw = dict(lanes_per_particle=lanes, rebuild_every=rebuild_every)
    st, got, info = _run(capi, prm, parts, [n_steps], **kw)
    assert info["tuning"]["lanes_per_particle"] == lanes, info
    if rebuild_every:
        assert info["policy"]["rebuild_every"] == rebuild_every, info
    else:
        assert info["sched"]["fuse_ea"] == 1 and info["policy"]["rebuild_every"] == 16, info
    assert info["sched_after"]["rebins"] - info["sched"]["rebins"] >= 1, info
    _same(f"{lanes} lanes K={rebuild_every}, second run", (st, got), _run(capi, prm, parts, [n_steps], **kw)[:2])
    ref = _oracle(oracle, prm, parts, n_steps)
    rs = ref["stats"]
    err = _errors(got, ref)
    with capsys.disabled():
        print(f"\n[leading arguments] {lanes} lanes K={rebuild_every} {n_steps} steps: max rel err "
              + " ".join(f"{k}={v:.1e}" for k, v in err.items())
              + f" | t {abs(st['t'] - rs['t']) / rs['t']:.1e} dt {abs(st['dt_last'] - rs['dt_last']) / rs['dt_last']:.1e}")
    assert st["step"] == n_steps == rs["steps"]
    assert abs(st["t"] - rs["t"]) <= 1e-12 * rs["t"]
    assert abs(st["dt_last"] - rs["dt_last"]) <= RTOL * rs["dt_last"]
    assert abs(st["vmax"] - rs["vmax"]) <= RTOL * rs["vmax"]
    for k, e in err.items():
        assert e <= RTOL, f"{lanes} lanes K={rebuild_every}:{k}: {e:.3e} > {RTOL:.0e}"


@pytest.mark.parametrize("lanes", [16, 32])
def test_phases_of_captured_graphs(lanes, cfgmod, geom, capi):
    prm, parts = _start(cfgmod, geom)
    kw = dict(lanes_per_particle=lanes)
    whole = _run(capi, prm, parts, [20], **kw)
    assert whole[0]["step"] == 20 and whole[2]["sched"]["fuse_ea"] == 1, whole[2]
    _same(f"{lanes} lanes, 7 + 13", whole[:2], _run(capi, prm, parts, [7, 13], **kw)[:2])  # the second graph starts mid-cycle
    _same(f"{lanes} lanes, twenty single steps", whole[:2], _run(capi, prm, parts, [1] * 20, **kw)[:2])  # eager launches


def test_dual_rate_packed_flag(cfgmod, geom, capi, capsys):
    prm, parts = _start(cfgmod, geom)
    kw = dict(lanes_per_particle=16, dual_rate=2)
    st, got, info = _run(capi, prm, parts, [6], **kw)
    assert info["substeps"] == 2 and info["tuning"]["lanes_per_particle"] == 16, info  # (pass CD with later = 1)
    _same("dual rate, second run", (st, got), _run(capi, prm, parts, [6], **kw)[:2])
    ref = dual_rate_reference.run(prm, parts, 2, max_outer=6)
    err = _errors(got, ref)
    with capsys.disabled():
        print("\n[leading arguments] dual rate, 16 lanes: max rel err " + " ".join(f"{k}={v:.1e}" for k, v in err.items()))
    assert st["step"] == ref["steps"] == 6 and abs(st["t"] - ref["t"]) <= 1e-12 * ref["t"]
    assert abs(st["dt_last"] - ref["dt_last"]) <= RTOL * ref["dt_last"]
    assert abs(st["vmax"] - ref["vmax"]) <= RTOL * ref["vmax"]
    for k, e in err.items():
        assert e <= RTOL, f"dual rate:{k}: {e:.3e} > {RTOL:.0e}"


def test_batch_members_are_standalone_contexts(cfgmod, geom, capi):
    starts = [_start(cfgmod, geom, seed) for seed in (21, 22, 23)]
    assert not np.array_equal(starts[0][1]["pos"], starts[1][1]["pos"])
    with capi.Batch.from_parts(*zip(*starts), t_end=1e9, lanes_per_particle=16) as b:
        sts = b.advance(1e9, max_steps=20)
        got = [b.download(m) for m in range(3)]
        assert b.info()["lanes_per_particle"] == 16 and b.info()["realignments"] == 0
    for m, (prm, parts) in enumerate(starts):
        st, ref, _ = _run(capi, prm, parts, [20], lanes_per_particle=16)
        assert sts[m]["step"] == st["step"] == 20
        for k in ("t", "dt_last", "vmax"):
            assert sts[m][k] == st[k], (m, k)
        for k, v in ref.items():
            assert np.array_equal(np.asarray(got[m][k]), v), f"member {m}: {k} differs"
