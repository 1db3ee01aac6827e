"""Shared test helpers: seeded inputs and tolerance checks."""
import numpy as np


def make_case(cfgmod, geom, dp=0.05, DL=3.0, seed=1234, jitter=0.2, developed=True, **kw):
    """Lattice + uniform jitter (+- jitter*dp) + (optionally) a developed-flow-like state:
    parabolic u_x, small random u_y, non-zero drho_dt.  Deterministic for a given seed."""
    prm = cfgmod.params_from_values(dp=dp, DL=DL, **kw)
    parts = geom.init_particles(prm)
    nf, nt = parts["n_fluid"], parts["n_total"]
    rng = np.random.default_rng(seed)
    pos = parts["pos"].copy(order="F")
    vel = parts["vel"].copy(order="F")
    drho = parts["drho_dt"].copy()
    if jitter:
        pos[:nf] += (rng.random((nf, 2)) * 2 - 1) * jitter * prm.dp
        pos[:nf, 0] = pos[:nf, 0] - np.floor(pos[:nf, 0] / prm.DL) * prm.DL
    if developed:
        y = pos[:nf, 1]
        vel[:nf, 0] = prm.gravity_g / (2 * prm.nu) * y * (prm.DH - y) * (1 + 0.02 * rng.standard_normal(nf))
        vel[:nf, 1] = 0.02 * rng.standard_normal(nf)
        drho[:nf] = 0.5 * rng.standard_normal(nf)
    parts = dict(parts)
    parts.update(pos=pos, vel=vel, drho_dt=drho)
    return prm, parts


def make_variant(cfgmod, geom, seed=1234, top_ux=0.8, bottom_ux=-0.3, uy_sigma=0.05, mass_spread=0.2, **kw):
    """make_case plus what the reference takes as plain arguments and make_case leaves at zero / uniform: moving walls and
    uneven mass.  Top wall u_x = top_ux, bottom wall u_x = bottom_ux (different sign and size), each times 1 + 0.05 U(-1,1)
    per wall particle, u_y = uy_sigma N(0,1) per wall particle: every wall particle has its own velocity and x != y, so an
    index or component mix-up shows.  The fluid rows of wall_vel, which nothing may read, hold decoys of order 3.  Mass is
    multiplied by 1 + mass_spread U(-1,1) per particle, walls included.  rho0, DH, mu, c_f, U_bulk, transport_coeff go
    through **kw to params_from_values as in make_case.  Deterministic for a given seed."""
    prm, parts = make_case(cfgmod, geom, seed=seed, **kw)
    nf, nt = parts["n_fluid"], parts["n_total"]
    rng = np.random.default_rng(seed + 7919)
    wv = np.zeros((nt, 2), order="F")
    top = parts["pos"][nf:, 1] > 0.5 * prm.DH
    wv[nf:, 0] = np.where(top, top_ux, bottom_ux) * (1 + 0.05 * (rng.random(nt - nf) * 2 - 1))
    wv[nf:, 1] = uy_sigma * rng.standard_normal(nt - nf)
    wv[:nf, 0] = 3.0 + 0.5 * rng.random(nf)
    wv[:nf, 1] = -3.0 - 0.5 * rng.random(nf)
    mass = parts["mass"] * (1 + mass_spread * (rng.random(nt) * 2 - 1))
    parts.update(wall_vel=wv, mass=mass)
    return prm, parts


def with_density_floor(parts, rows=(3, 40), drho=-1e6):
    """A copy of parts whose drho_dt drives rho + dt/2 drho_dt of a few fluid particles below 1e-10 on the next step: the
    reference then takes rho0 for the half-step density (sph_physics_mex.c, `if (rho_half < 1e-10)`), so p = 0 there."""
    out = dict(parts, drho_dt=np.array(parts["drho_dt"], copy=True))
    out["drho_dt"][list(rows)] = drho
    return out


def canon_pairs(nb):
    """Sort a pair list by (i, j) so two lists can be compared as sets."""
    pi, pj = nb[0].astype(np.int64), nb[1].astype(np.int64)
    order = np.lexsort((pj, pi))
    return tuple(np.asarray(c)[order] for c in nb)


def assert_close(a, b, rtol=1e-11, atol_scale=1e-13, name="", atol=0.0):
    """|a-b| <= rtol*|b| + atol_scale*max|b| + atol element-wise.  The HIP kernels use the reference's
    formulas; differences come from summation order / FMA contraction only."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, f"{name}: shape {a.shape} vs {b.shape}"
    assert np.all(np.isfinite(a)), f"{name}: non-finite values"
    scale = np.max(np.abs(b)) if b.size else 0.0
    err = np.abs(a - b)
    tol = rtol * np.abs(b) + atol_scale * max(scale, 1e-300) + atol + 1e-300
    bad = err > tol
    assert not np.any(bad), (f"{name}: {int(bad.sum())}/{a.size} elements differ, max err {err.max():.3e} "
                             f"(scale {scale:.3e}, atol {atol:.1e}) at {np.argwhere(bad)[:3].tolist()}")


def field_atol(prm, parts, nb, dt):
    """Absolute round-off floors per field.  The weakly-compressible EOS p = p0 (rho/rho0 - 1) with
    p0 = rho0 c_f^2 turns a 1-ulp density difference into p0*eps of pressure, which then propagates into
    force, velocity and drho_dt sums that may cancel to ~0 (e.g. on the pristine lattice).  Floors are
    1e3 ulps of that chain -- ten orders of magnitude below any formula error."""
    eps = 2.3e-16 * 1e3
    dWV = float(np.max(np.abs(nb[6]))) * float(np.max(parts["mass"])) / prm.rho0 if len(nb[6]) else 1.0
    m = float(np.min(parts["mass"]))
    vol = float(np.max(parts["mass"])) / prm.rho0
    vmax = max(float(np.max(np.abs(parts["vel"]))), float(np.max(np.abs(parts["wall_vel"][parts["n_fluid"]:]), initial=0.0)))
    vmax += prm.gravity_g * dt
    a_rho = eps * prm.rho0
    a_p = eps * prm.p0
    a_F = 30 * dWV * vol * (a_p + eps * prm.mu * vmax / prm.h)
    a_v = a_F / m * dt + eps * vmax
    a_drho = 30 * dWV * prm.rho0 * (a_v + eps * vmax)
    return dict(rho=a_rho + 0.5 * dt * a_drho, p=a_p + prm.p0 / prm.rho0 * 0.5 * dt * a_drho, force=a_F,
                force_prior=a_F, vel=a_v, drho=a_drho, drho_dt=a_drho, pos=eps * prm.DL + dt * a_v, Vol=eps * vol,
                B=1e-12, zeros=0.0)
