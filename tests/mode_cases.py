"""Cases, bounds and comparisons shared by tests/test_modes_host.py, tests/test_gpu_modes.py, tests/test_gpu_batch_modes.py and
tests/test_matlab_modes.py (mode amplitudes, include/sphx.h sections 2t / 2u).

The bound of the GPU comparisons.  A summed field is compared with numpy's (profile.mode_sums) counter by counter, relative to
that field's sum of |q_i| over the particles -- not to the sum itself, which cancels to ~0 for most modes -- within
    BOUND = max(16 * FP_DEVIATION, 1e-12)   plus the quantisation term N * 2^-(s+1) of that field's scale,
the conventions of tests/dens_stats_cases.py.  FP_DEVIATION is the rounding error of the reference itself: the largest
deviation, over the jittered parabola at dp = 0.05 and 0.025 and all 17 x 17 modes, of the float64 definition from the same in
np.longdouble, in units of sum |q_i|.  MEASURED (tests/test_modes_host.py::test_floating_point_bound prints it and asserts it
stays below the constant): 3.0e-16 at dp = 0.05 (uy), 2.1e-16 at dp = 0.025 (ux); the constant is rounded up to 5e-16.  16 x is for the
device's different arithmetic (sincospi and a rotation recurrence against numpy's cos(m theta): up to 16 turns of 1.1e-16 each,
and an argument m theta that numpy rounds before it takes the cosine), and 16 * 5e-16 = 8e-15 < 1e-12: the floor, the field
map's bound, is what holds.  The quantisation term is derived, not measured: a particle's term is rounded to the nearest
multiple of 2^-s, so a sum over N particles is off by at most N * 2^-(s+1).

The exact identities hold bit for bit on the host and on the device: n[0, 0, cc] = N, every sc / ss sum of m = 0 and every
cs / ss sum of n = 0 is 0 (cos 0 = 1 and sin 0 = 0 exactly)."""
import numpy as np

import probe_cases

CASES = probe_cases.CASES      # compact, walk, dynamic and dual-rate forms, two columns, one column, 30 k particles, a wide skin
MODES = ((0, 0), (4, 8), (16, 16))  # one counter set in one group; the default; the limits (289 modes, 3 468 counters)
FIELDS = ("n", "ux", "uy")
BASES = ("cc", "sc", "cs", "ss")
SERIES = ("step", "t") + FIELDS
SCALE_OF = dict(n="s0", ux="s1", uy="s1")
FP_DEVIATION = 5e-16
BOUND = max(16 * FP_DEVIATION, 1e-12)
BLOCK = 256                    # threads of a workgroup of k_modes (csrc/sphx_modes.hpp, kModesBlock)
CHUNK = 8 * BLOCK              # particles up to which the sample has one chunk (kModesPerThread * kModesBlock): with modes
                               # (0, 0) -- one group -- ONE workgroup finishes it alone, no global sums, no ticket
RUN = 3                        # consecutive n a workgroup serves (kModesRun): ny = 2 is one group per m, ny = 3 two

# Start-up of plane Poiseuille flow from rest, dp = 0.05, DL = 3, to t = 0.4 (374 steps): the largest distance of b_n(t) =
# (2 / N) ux[0, n, cs] from the closed form profile.mode_b_exact over the steps, in U_max, of the ORACLE's own trajectory
# (oracle.run chained step by step, profile.mode_sums of every state).  MEASURED on the CPU by
# tests/test_modes_host.py::test_startup_distance_of_the_oracle, which prints them and asserts these constants.
STARTUP = dict(dp=0.05, DL=3.0, t_end=0.4)
STARTUP_DISTANCE = {1: 5.4033e-4, 3: 6.5443e-4}
STARTUP_MARGIN = 1.5           # for summation order only
PARITY = 1e-10                 # the suite's parity tolerance against the oracle (tests/test_gpu_resident.py: 1e-10 of a field's scale)


def case(maker, cfgmod, geom, name, seed=11):
    return probe_cases.case(maker, cfgmod, geom, name, seed)


def numpy_modes(profmod, prm, pos_fluid, vel_fluid, mx, ny, acc=np.float64):
    return profmod.mode_sums(pos_fluid, vel_fluid, prm.DL, prm.DH, mx, ny, acc=acc)


def deviation(a, b):
    """(largest deviation of a counter between two mode_sums dicts, in units of the field's sum |q_i| of b; the field)"""
    worst = (0.0, None)
    for f in FIELDS:
        scale = b["abs_" + f]
        if scale > 0.0:
            worst = max(worst, (float(np.max(np.abs(a[f] - b[f]))) / scale, f), key=lambda w: w[0])
    return worst


def assert_exact_identities(rec, n_particles, what):
    """one record {n, ux, uy: [mx + 1, ny + 1, 4]}: the identities that hold to the bit"""
    assert rec["n"][0, 0, 0] == float(n_particles), f"{what}: n[0, 0, cc] = {rec['n'][0, 0, 0]!r}, N = {n_particles}"
    for f in FIELDS:
        v = np.asarray(rec[f])
        assert np.all(v[0, :, 1] == 0.0) and np.all(v[0, :, 3] == 0.0), f"{what}: {f}: a sine sum of m = 0 is not 0"
        assert np.all(v[:, 0, 2] == 0.0) and np.all(v[:, 0, 3] == 0.0), f"{what}: {f}: a sine sum of n = 0 is not 0"


def record(series, r):
    return {f: np.asarray(series[f])[r] for f in FIELDS}


def assert_record_matches(rec, want, scales, n_particles, what, bound=BOUND):
    """one record against profile.mode_sums of the same state: every counter within bound of the field's sum |q_i| plus the
    quantisation term N * 2^-(s+1) of profile.mode_scales, and the exact identities"""
    assert_exact_identities(rec, n_particles, what)
    for f in FIELDS:
        got, ref = np.asarray(rec[f], dtype=np.float64), np.asarray(want[f], dtype=np.float64)
        assert got.shape == ref.shape, f"{what}: {f} {got.shape} {ref.shape}"
        quant = n_particles * 2.0 ** -(scales[SCALE_OF[f]] + 1)
        allowed = bound * want["abs_" + f] + quant
        err = float(np.max(np.abs(got - ref)))
        print(f"{what}: {f} off by {err / max(want['abs_' + f], 1e-300):.3e} of sum |q| {want['abs_' + f]:.3e}, quantisation {quant:.3e}")
        assert np.all(np.isfinite(got)) and err <= allowed, f"{what}: {f} off by {err:.3e}, allowed {allowed:.3e}"


def assert_series_identical(a, b, what, counters=True):
    """two modes dicts byte for byte"""
    for k in SERIES:
        assert np.asarray(a[k]).shape == np.asarray(b[k]).shape, f"{what}: {k} {np.asarray(a[k]).shape} {np.asarray(b[k]).shape}"
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), f"{what}: {k}"
    if counters:
        assert a["n_dropped"] == b["n_dropped"], what


def oracle_trajectory(oracle, prm, parts, t_end):
    """the oracle's loop from the state of parts to t_end, one call per step, each continuing the last (bit for bit one call
    of all the steps): -> t [n], and the fluid rows pos, vel [n, N, 2] after every step"""
    nf = parts["n_fluid"]
    st, t, step = {}, 0.0, 0
    ts, ps, vs = [], [], []
    while t < t_end - 1e-12:
        r = oracle.run(prm, parts, t_end=t_end, output_interval=1e9, max_steps=1, enable_sort=False, t0=t, step0=step, **st)
        st = dict(pos=r["pos"], vel=r["vel"], drho_dt=r["drho_dt"])
        t, step = r["stats"]["t"], step + 1
        ts.append(t)
        ps.append(r["pos"][:nf].copy())
        vs.append(r["vel"][:nf].copy())
    return np.array(ts), np.array(ps), np.array(vs)


def b_series(profmod, prm, pos, vel, ns=(1, 3)):
    """{n: b_n [n_records]} = (2 / N) ux[0, n, cs] of profile.mode_sums of every state of a trajectory"""
    top = max(ns)
    S = [profmod.mode_sums(p, v, prm.DL, prm.DH, 0, top)["ux"] for p, v in zip(pos, vel)]
    return {n: np.array([2.0 / len(p) * s[0, n, 2] for s, p in zip(S, pos)]) for n in ns}
