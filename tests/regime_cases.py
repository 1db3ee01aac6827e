"""States that enter the branches of the step which the suite's default states never reach, and a census that proves it.

The default states (helpers.make_case / make_variant with config.py's physics) flow to the right, stay far below the cap of the
Riemann dissipation and are limited by the acoustic dt on every step.  The cases here mirror the flow (left crossings of the
periodic seam), lower c_f until many pairs reach the cap fmin(3 max(du, 0), c_f), raise mu until the viscous dt binds, raise
|g| until the body dt binds, and drive two rows through the density floor.  census() measures, with the oracle and numpy
alone, that a case does what it is for; tests/test_regime_cases.py asserts it, so a case cannot silently stop doing its job.

Shared by tests/test_regime_cases.py, test_reference_anchor.py, test_gpu_regimes.py, test_gpu_mex_surface.py and the switch
workers.  A plain module: no fixtures."""
import dataclasses

import numpy as np

from helpers import make_case, make_variant, with_density_floor

# dp, jitter and seed of the two sizes: test_gpu_resident's small state and tests/switch_worker.py's state
SIZES = {"small": dict(dp=0.05, DL=1.5, jitter=0.2, seed=7), "worker": dict(dp=0.025, DL=1.5, jitter=0.25, seed=31)}
LEFT = dict(U_bulk=-0.666667)
MIRRORED_WALLS = dict(top_ux=-0.8, bottom_ux=0.3, rho0=2.5, transport_coeff=0.1)  # make_variant's walls, mirrored
FLOOR_ROWS = (3, 40)


def default(cfgmod, geom, size):
    """The suite's own state: what the regime cases are the opposite of."""
    return make_case(cfgmod, geom, developed=True, **SIZES[size])


def leftward_plain(cfgmod, geom, size):
    """make_case with U_bulk < 0: fixed walls, so it can share a batch's or a sampler test's walls."""
    return make_case(cfgmod, geom, developed=True, **SIZES[size], **LEFT)


def leftward(cfgmod, geom, size):
    return make_variant(cfgmod, geom, developed=True, **SIZES[size], **LEFT, **MIRRORED_WALLS)


def capped(cfgmod, geom, size):
    return make_case(cfgmod, geom, developed=True, **SIZES[size], c_f=0.3)


def left_capped(cfgmod, geom, size):
    return make_variant(cfgmod, geom, developed=True, **SIZES[size], **LEFT, **MIRRORED_WALLS, c_f=0.3)


def viscous(cfgmod, geom, size):
    return make_variant(cfgmod, geom, developed=True, **SIZES[size], mu=2.0, rho0=2.5, transport_coeff=0.1)


def viscous_plain(cfgmod, geom, size):
    return make_case(cfgmod, geom, developed=True, **SIZES[size], mu=2.0)


def body(cfgmod, geom, size):
    """At rest under g = -100: body-limited first, acoustic once the fluid has sped up (to the left)."""
    prm, parts = make_case(cfgmod, geom, developed=False, **SIZES[size], c_f=1.0, mu=0.01)
    return dataclasses.replace(prm, gravity_g=-100.0), parts


def floor(cfgmod, geom, size):
    """Moving walls, rho0 = 2.5, and a drho_dt of -1e6 on FLOOR_ROWS: their half-step density falls below 1e-10 on the first
    step and the reference takes rho0 instead (sph_physics_mex.c, `if (rho_half < 1e-10)`)."""
    kw = dict(SIZES[size], seed=109) if size == "small" else SIZES[size]
    prm, parts = make_variant(cfgmod, geom, **kw, rho0=2.5, transport_coeff=0.1)
    return prm, with_density_floor(parts, rows=FLOOR_ROWS)


CASES = {"leftward": leftward, "capped": capped, "left_capped": left_capped, "viscous": viscous, "body": body, "floor": floor}


def dt_viscous(prm):
    return 0.125 * prm.h * prm.h / max(prm.nu, 1e-12)


def dt_body(prm):
    return 0.25 * np.sqrt(prm.h / max(abs(prm.gravity_g), 1e-12))


def pair_classes(prm, parts, oracle, pos=None, vel=None):
    """Fluid-fluid pairs by where the Riemann dissipation fmin(3 max(du, 0), c_f) puts them, du = (v_i - v_j) . e with e the
    unit vector of the pair's (dx, dy): zero (du <= 0), linear (0 < du < c_f / 3) and capped (du >= c_f / 3)."""
    nf, nt = parts["n_fluid"], parts["n_total"]
    pos = parts["pos"] if pos is None else pos
    vel = parts["vel"] if vel is None else vel
    pi, pj, dx, dy, r, _, _ = oracle.neighbor_search(pos, nf, nt, prm.h, prm.DL)
    i, j = pi.astype(np.int64) - 1, pj.astype(np.int64) - 1
    ff = (i < nf) & (j < nf) & (r > 0)
    i, j = i[ff], j[ff]
    du = ((vel[i, 0] - vel[j, 0]) * dx[ff] + (vel[i, 1] - vel[j, 1]) * dy[ff]) / r[ff]
    per_row = np.bincount(np.concatenate([i, j]), minlength=nf) if len(i) else np.zeros(nf, dtype=np.int64)
    return dict(zero=int(np.count_nonzero(du <= 0.0)), linear=int(np.count_nonzero((du > 0.0) & (du < prm.c_f / 3.0))),
                capped=int(np.count_nonzero(du >= prm.c_f / 3.0)), total=int(len(du)), du_max=float(np.max(du, initial=0.0)),
                max_neighbours=int(np.max(per_row, initial=0)))


def census(prm, parts, oracle, n_steps):
    """What the oracle's n_steps from this state pass through, one step at a time:
      pairs_start, pairs_end   pair_classes of the first and the last state
      limits                   one letter per step for the limit that bound dt: A(coustic), V(iscous), B(ody); '?' if none
      left, right              seam crossings: x jumped by more than DL / 2 up (left the channel at x < 0) or down
      floored                  the rows whose half-step density the first step floored (see floored_rows)
      dt, vmax, rho_range, finite   the dt series, the last step's vmax, min and max of rho / rho0 over the run, all finite"""
    nf = parts["n_fluid"]
    pos, vel, drho = parts["pos"], parts["vel"], parts["drho_dt"]
    t, limits, dts, left, right, floored = 0.0, "", [], 0, 0, []
    rho_lo, rho_hi, finite = np.inf, -np.inf, True
    out = dict(pairs_start=pair_classes(prm, parts, oracle))
    st = None
    for k in range(n_steps):
        v = np.sqrt(vel[:nf, 0] ** 2 + vel[:nf, 1] ** 2)
        x0 = pos[:nf, 0].copy()
        st = oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=1, enable_sort=False, pos=pos, vel=vel,
                        drho_dt=drho, t0=t, step0=k)
        dt = st["stats"]["dt_last"]
        near = lambda want: abs(dt - want) <= 1e-13 * want
        limits += ("V" if near(dt_viscous(prm)) else "B" if near(dt_body(prm)) else
                   "A" if near(0.25 * prm.h / max(prm.c_f + float(np.max(v, initial=0.0)), 1e-12)) else "?")
        dts.append(dt)
        if k == 0:
            floored = floored_rows(prm, st, nf)
        pos, vel, drho, t = st["pos"], st["vel"], st["drho_dt"], st["stats"]["t"]
        jump = pos[:nf, 0] - x0
        left += int(np.count_nonzero(jump > 0.5 * prm.DL))
        right += int(np.count_nonzero(jump < -0.5 * prm.DL))
        finite = finite and all(bool(np.all(np.isfinite(st[f]))) for f in ("pos", "vel", "rho", "p", "drho_dt", "force"))
        rho_lo, rho_hi = min(rho_lo, float(np.min(st["rho"][:nf]))), max(rho_hi, float(np.max(st["rho"][:nf])))
    out.update(pairs_end=pair_classes(prm, parts, oracle, pos, vel), limits=limits, left=left, right=right, floored=floored,
               dt=np.array(dts), vmax=float(st["stats"]["vmax"]) if st else 0.0,
               rho_range=(rho_lo / prm.rho0, rho_hi / prm.rho0), finite=finite, last=st)
    return out


def floored_rows(prm, state, n_fluid, ulps=0):
    """The fluid rows of a state one step after its start whose half-step density was floored.  A step ends with
    rho = rho_half + drho_dt dt / 2 and p = p0 (rho / rho0 - 1) (sph_physics_mex.c:1429-1451), so the step's p is 0 only where
    drho_dt is; what a floored row shows is rho == rho0 + drho_dt dt / 2 with the constant rho0 for rho_half, which no row
    reaches by summation (the summed density of a jittered lattice plus dt / 2 of a drho_dt is never rho0 to the last bit).
    ulps > 0 allows that many of rho0 for a device that contracts the closing update into a fused multiply-add."""
    dt = state["stats"]["dt_last"] if "stats" in state else state["dt_last"]
    want = prm.rho0 + state["drho_dt"][:n_fluid] * (0.5 * dt)
    return [int(i) for i in np.flatnonzero(np.abs(state["rho"][:n_fluid] - want) <= ulps * np.spacing(prm.rho0))]
