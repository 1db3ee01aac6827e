"""-m gpu: the compact kernels at 16 and 32 lanes per particle with their rows requested ahead (sphx_kernels.hpp, kRowsAhead).

Passes B, CD and E request the neighbour records of a lane's rows 0 and 1 in one wave and walk rows 2 and up in a remainder loop;
pass A's walk of the superset list does the same with its first P = 64 / lanes rows (four at 16 lanes).  The second wall loop of
pass CD takes the wall rows among the prefetched ones from registers and reads the others again.  Each case below puts lanes on
one side or the other of these thresholds -- and asserts, with a brute-force count on the CPU, that it does.

Channel: dp = 0.05, DL = 1.5, DH = 1 -- 600 fluid particles in seven cell columns, so the re-binning step is the folded one
(k_forces_hist, k_continuity_rebin); at 16 lanes per particle 37.5 workgroups: a partial last workgroup and both branches of
xcd_block.  Start: geometry.developed_state with a jitter of 0.2 dp (row counts differ from lane to lane); 20 steps cross the
scheduled re-binning of step 16.

Reference and tolerances: oracle.run on the same state, the nine fields, t, dt and max |v| as tests/test_gpu_headline_parity.py
compares them, at that file's bound for 20 steps (RTOL[20] = 1e-10 in max|a - b| / max|b| per field: the two sides evaluate the
same formulas in a different summation order).  The dual-rate loop is not the reference's loop; its reference is
tests/dual_rate_reference.py, the oracle's functions composed into outer steps and inner sub-steps (more cases of it:
tests/test_gpu_dual_rate_parity.py).  Its case compares 16 lanes per particle with 32 -- the same formulas, the rows dealt
differently over the lanes, so again a different summation order -- and each of the two with that reference, all at the same
bound.  Every case also runs twice and must repeat to the bit.
"""
import numpy as np
import pytest

import dual_rate_reference

pytestmark = pytest.mark.gpu

FIELDS = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B")
RTOL = 1e-10  # tests/test_gpu_headline_parity.py, RTOL[20]
N_STEPS = 20
DP, DL = 0.05, 1.5


def _start(cfgmod, geom, squeeze=None):
    prm = cfgmod.params_from_values(dp=DP, DL=DL)
    parts = dict(geom.init_particles(prm))
    pos, vel = geom.developed_state(prm, parts, jitter=0.2, seed=21)
    nf = parts["n_fluid"]
    assert nf == 600 and abs(prm.DH - 1.0) < 1e-12
    if squeeze is not None:  # (centre, radius, factor): the fluid inside the circle moves towards its centre
        c, radius, factor = squeeze
        d = pos[:nf] - np.asarray(c)
        inside = np.hypot(d[:, 0], d[:, 1]) < radius
        pos[:nf][inside] = np.asarray(c) + factor * d[inside]
    parts.update(pos=pos, vel=vel)
    return prm, parts


def _counts_within(prm, parts, radius):
    """Per fluid particle: how many particles (fluid or wall) lie within `radius`, itself excluded, with the minimum image in x;
    and how many of them are wall particles."""
    nf = parts["n_fluid"]
    p = np.asarray(parts["pos"])
    dx = p[:nf, None, 0] - p[None, :, 0]
    dx -= prm.DL * np.round(dx / prm.DL)
    dy = p[:nf, None, 1] - p[None, :, 1]
    r2 = dx * dx + dy * dy
    near = (r2 < radius * radius) & (r2 > 1e-24)
    return near.sum(axis=1), near[:, nf:].sum(axis=1)


def _run(capi, prm, parts, n_steps=N_STEPS, **kw):
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        info = dict(tuning=ctx.tuning(), policy=ctx.grid_policy(), sched=ctx.schedule(), substeps=ctx.substeps())
        st = ctx.advance(1e9, max_steps=n_steps)
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


def _check_against_oracle(name, capi, oracle, capsys, prm, parts, lanes, **kw):
    st, got, info = _run(capi, prm, parts, lanes_per_particle=lanes, **kw)
    st2, got2, _ = _run(capi, prm, parts, lanes_per_particle=lanes, **kw)
    assert info["tuning"]["lanes_per_particle"] == lanes, info
    assert info["sched"]["fuse_ea"] == 1, info
    assert info["sched_after"]["rebins"] - info["sched"]["rebins"] >= 1, info  # the folded re-binning step was crossed
    assert st == st2
    for k, v in got.items():
        assert np.array_equal(v, got2[k]), f"{name}: {k} differs between two runs"
    ref = oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=N_STEPS, enable_sort=False)
    rs = ref["stats"]
    assert st["step"] == N_STEPS == rs["steps"]
    err = _errors(got, ref)
    with capsys.disabled():
        print(f"\n[load chains] {name}: max rel err " + " ".join(f"{k}={v:.1e}" for k, v in err.items())
              + f" | t {abs(st['t'] - rs['t']) / rs['t']:.1e} dt {abs(st['dt_last'] - rs['dt_last']) / rs['dt_last']:.1e}")
    assert abs(st["t"] - rs["t"]) <= 1e-12 * rs["t"]
    assert abs(st["dt_last"] - rs["dt_last"]) <= RTOL * rs["dt_last"]
    assert abs(st["vmax"] - rs["vmax"]) <= RTOL * rs["vmax"]
    for k, e in err.items():
        assert e <= RTOL, f"{name}:{k}: {e:.3e} > {RTOL:.0e}"
    return info


def test_32_lanes_one_row_or_none(cfgmod, geom, capi, oracle, capsys):
    prm, parts = _start(cfgmod, geom)
    n_all, _ = _counts_within(prm, parts, 2.0 * prm.h)
    assert n_all.max() <= 32 and n_all.min() < 32  # no lane owns a second row of the step's list, many own none
    _check_against_oracle("32 lanes", capi, oracle, capsys, prm, parts, 32)


def test_16_lanes_default_skin(cfgmod, geom, capi, oracle, capsys):
    prm, parts = _start(cfgmod, geom)
    n_all, _ = _counts_within(prm, parts, 2.0 * prm.h)
    assert 16 < n_all.max() <= 32  # one to two rows in passes B, CD and E
    info = _check_against_oracle("16 lanes", capi, oracle, capsys, prm, parts, 16)
    n_sup, _ = _counts_within(prm, parts, 2.0 * prm.h + info["policy"]["skin"])
    assert 32 < n_sup.max() <= 64, n_sup.max()  # three to four rows in pass A's walk, none behind the prefetched ones


def test_16_lanes_superset_rows_beyond_the_prefetched(cfgmod, geom, capi, oracle, capsys):
    prm, parts = _start(cfgmod, geom)
    skin_h = None
    for s in (1.5, 1.75, 2.0, 2.25, 2.5):  # raised until some particle has more than P * 16 = 64 candidates within 2h + skin
        if _counts_within(prm, parts, (2.0 + s) * prm.h)[0].max() > 64:
            skin_h = s
            break
    assert skin_h is not None
    info = _check_against_oracle(f"16 lanes, skin {skin_h} h", capi, oracle, capsys, prm, parts, 16, skin_h=skin_h,
                                 rebuild_every=16)
    assert abs(info["policy"]["skin"] - skin_h * prm.h) <= 1e-12 and info["policy"]["rebuild_every"] == 16, info
    assert _counts_within(prm, parts, 2.0 * prm.h + info["policy"]["skin"])[0].max() > 64  # pass A's remainder loop has run


def test_16_lanes_more_than_two_rows_with_wall_rows_among_them(cfgmod, geom, capi, oracle, capsys):
    # the fluid within 4.5 dp of a point one spacing above the bottom wall, drawn together to 0.7 of its distances
    prm, parts = _start(cfgmod, geom, squeeze=((0.75, 1.0 * DP), 4.5 * DP, 0.7))
    n_all, n_wall = _counts_within(prm, parts, 2.0 * prm.h)
    # more than 2 * 16 true neighbours: the remainder loops of passes B, CD and E; wall neighbours stand last in a list, so with
    # walls among more than 32 the entries from the 33rd on are wall entries: the second wall loop reads rows again
    assert n_all.max() > 32
    assert np.any((n_all > 32) & (n_wall > 0))
    _check_against_oracle("16 lanes, squeezed", capi, oracle, capsys, prm, parts, 16)


def test_dual_rate_16_lanes_against_32(cfgmod, geom, capi, oracle, capsys):
    prm, parts = _start(cfgmod, geom)
    ref = dual_rate_reference.run(prm, parts, 2, max_outer=6)
    out = {}
    for lanes in (16, 32):
        st, got, info = _run(capi, prm, parts, n_steps=6, lanes_per_particle=lanes, dual_rate=2)
        st2, got2, _ = _run(capi, prm, parts, n_steps=6, lanes_per_particle=lanes, dual_rate=2)
        assert info["substeps"] == 2 and info["tuning"]["lanes_per_particle"] == lanes, info  # (pass CD with later = 1)
        assert st["step"] == 6 and st == st2
        for k, v in got.items():
            assert np.array_equal(v, got2[k]), f"dual rate, {lanes} lanes: {k} differs between two runs"
        out[lanes] = (st, got)
    (sa, a), (sb, b) = out[16], out[32]
    err = _errors(a, b)
    with capsys.disabled():
        print("\n[load chains] dual rate, 16 against 32 lanes: max rel err " + " ".join(f"{k}={v:.1e}" for k, v in err.items()))
    assert abs(sa["t"] - sb["t"]) <= 1e-12 * sb["t"]
    assert abs(sa["dt_last"] - sb["dt_last"]) <= RTOL * sb["dt_last"]
    for k, e in err.items():
        assert e <= RTOL, f"dual rate:{k}: {e:.3e} > {RTOL:.0e}"
    for lanes, (st, got) in out.items():  # ... and each of them against the reference of the dual-rate loop
        err = _errors(got, ref)
        with capsys.disabled():
            print(f"[load chains] dual rate, {lanes} lanes against the reference: max rel err "
                  + " ".join(f"{k}={v:.1e}" for k, v in err.items()))
        assert st["step"] == ref["steps"] == 6 and abs(st["t"] - ref["t"]) <= 1e-12 * ref["t"]
        assert abs(st["dt_last"] - ref["dt_last"]) <= RTOL * ref["dt_last"]
        assert abs(st["vmax"] - ref["vmax"]) <= RTOL * ref["vmax"]
        for k, e in err.items():
            assert e <= RTOL, f"dual rate, {lanes} lanes against the reference:{k}: {e:.3e} > {RTOL:.0e}"
