"""CPU reference of the opt-in dual-rate loop (sphx_params.dual_rate in include/sphx.h; Clock::n_in, next_dt and forces_pass
"later" in sphx_kernels.hpp), composed from the oracle's functions -- each of them anchored to the reference's own C by
tests/test_oracle_anchor.py and tests/test_reference_anchor.py.  TEST INFRASTRUCTURE ONLY; nothing here calls libsphx.

One OUTER step is the reference's step (SPH_Poiseuille.m:250-292, oracle.run) with its acoustic part taken n_in times:

  1. nb = neighbor_search(pos); rho, Vol, B = density_correction(nb); fp = viscous_force(nb, vel, Vol, B) + mass g on the x
     component of the fluid rows, zero on the wall rows; pos = transport_correction(nb, Vol, B, pos).
  2. vmax = max |v| over the fluid; remain = min(t_target - t, t_end - t);
     Dt = min(0.25 h / max(vmax, 1e-12), dt_viscous, dt_body, remain, n_in 0.25 h / max(c_f + vmax, 1e-12));
     dt = max(Dt / n_in, 1e-12), with dt_viscous = 0.125 h^2 / nu and dt_body = 0.25 sqrt(h / |g|) as oracle.verlet_time_step.
  3. n_in times: integration_verlet with the SAME nb (so the pair geometry dx, dy, r, dW of step 1), Vol, B and fp, and the rho,
     pos, vel, drho_dt it returned last; then x wrapped periodically and the wall rows of vel set to zero.
  4. t += n_in dt.

With n_in = 1 this is oracle.run to the bit (tests/test_dual_rate_reference.py).  Rows stay in input order: nothing sorts.
"""
import math

import numpy as np

import oracle as orc  # oracle/oracle.py; tests/conftest.py puts its directory on sys.path

FIELDS = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B")
DP, DL = 0.05, 1.5
SQUEEZE_CENTRES = dict(bottom=(0.75, DP), top=(0.75, 1.0 - DP), seam=(0.0, DP))  # DH = 1 at the default parameters

# Deliberately wrong loops, for the test that shows this reference can tell them from the right one (`wrong=` below):
#   research    pairs searched again before every inner sub-step after the first
#   fp          force_prior computed again (from the carried velocity) before every inner sub-step after the first
#   stale_drho  every inner sub-step starts from the drho_dt of the outer step's start
#   vel_prev    the velocity after sub-step n_in - 1 is handed on in place of the last one
WRONG = ("research", "fp", "stale_drho", "vel_prev")


def substeps(prm, dual_rate):
    """Inner sub-steps per outer step of a context that asked for `dual_rate` and is eligible: as many acoustic steps (at
    max |v| = 0.1 c_f) as fit into the viscous / body-force step, at most dual_rate."""
    if dual_rate <= 1:
        return 1
    nu = prm.mu / prm.rho0
    dt_viscous = 0.125 * prm.h * prm.h / max(nu, 1e-12)
    dt_body = 0.25 * math.sqrt(prm.h / max(abs(prm.gravity_g), 1e-12))
    dt_acoustic = 0.25 * prm.h / (1.1 * prm.c_f)
    return max(1, min(int(math.floor(min(dt_viscous, dt_body) / dt_acoustic)), int(dual_rate)))


def _vmax(vel, nf):
    vx, vy = vel[:nf, 0], vel[:nf, 1]
    return float(np.max(np.sqrt(vx * vx + vy * vy))) if nf else 0.0


def outer_dt(prm, vmax, n_in, remain):
    """-> the inner step dt of an outer step that starts with max |v| = vmax and `remain` left to its target."""
    h = prm.h
    nu = prm.mu / prm.rho0
    dt_viscous = 0.125 * h * h / max(nu, 1e-12)
    dt_body = 0.25 * math.sqrt(h / max(abs(prm.gravity_g), 1e-12))
    dt_adv = 0.25 * h / max(vmax, 1e-12)
    dt_acoustic = 0.25 * h / max(prm.c_f + vmax, 1e-12)
    Dt = min(dt_adv, dt_viscous, dt_body, remain, n_in * dt_acoustic)
    return max(Dt / n_in, 1e-12)


def first_outer_step(prm, parts, n_in):
    """Length Dt = n_in dt of the first outer step from `parts` when no target clips it."""
    return n_in * outer_dt(prm, _vmax(np.asarray(parts["vel"]), parts["n_fluid"]), n_in, 1e9)


def run(prm, parts, n_in, t_target=1e9, t_end=1e9, max_outer=0, state=None, wrong=None):
    """Outer steps while t < t_target - 1e-12 and fewer than max_outer (> 0) were taken by this call.  -> dict of the nine
    FIELDS in input row order, t, dt_last, vmax (after the last step), steps (outer steps since t = 0, earlier calls included).
    state: the result of an earlier call, to go on from; parts gives mass and wall_vel either way."""
    assert n_in >= 1 and (wrong is None or wrong in WRONG)
    nf, nt = parts["n_fluid"], parts["n_total"]
    mass = np.asarray(parts["mass"], dtype=np.float64)
    wall_vel = np.asarray(parts["wall_vel"], dtype=np.float64)
    src = parts if state is None else state
    pos = np.array(src["pos"], dtype=np.float64, order="F")
    vel = np.array(src["vel"], dtype=np.float64, order="F")
    drho_dt = np.array(src["drho_dt"], dtype=np.float64)
    t, steps, dt = (0.0, 0, 0.0) if state is None else (float(state["t"]), int(state["steps"]), float(state["dt_last"]))
    out = {k: np.array(state[k], copy=True) for k in FIELDS} if state is not None else None
    t_target = min(t_target, t_end)
    taken = 0
    while t < t_target - 1e-12 and not (max_outer > 0 and taken >= max_outer):
        nb = orc.neighbor_search(pos, nf, nt, prm.h, prm.DL)
        rho, Vol, B = orc.density_correction(nb, mass, nf, nt, prm.rho0, prm.h, prm.inv_sigma0)

        def force_prior(nb_, vel_):
            f = orc.viscous_force(nb_, vel_, Vol, B, prm.mu, prm.h, nf, nt, mass, wall_vel)
            f[:nf, 0] += mass[:nf] * prm.gravity_g
            f[nf:] = 0.0
            return f

        fp = force_prior(nb, vel)
        pos = orc.transport_correction(nb, Vol, B, pos, prm.h, nf, nt, prm.transport_coeff)
        dt = outer_dt(prm, _vmax(vel, nf), n_in, min(t_target - t, t_end - t))
        drho_outer, vel_before_last = drho_dt, vel
        for m in range(n_in):
            if m and wrong == "research":
                nb = orc.neighbor_search(pos, nf, nt, prm.h, prm.DL)
            if m and wrong == "fp":
                fp = force_prior(nb, vel)
            vel_before_last = vel
            rho, p, pos, vel, drho_dt, force = orc.integration_verlet(
                nb, Vol, B, rho, mass, pos, vel, drho_outer if wrong == "stale_drho" else drho_dt, fp, dt, nf, nt,
                prm.rho0, prm.p0, prm.c_f, wall_vel)
            pos[:nf, 0] = pos[:nf, 0] - np.floor(pos[:nf, 0] / prm.DL) * prm.DL
            vel[nf:] = 0.0
        if wrong == "vel_prev" and n_in > 1:
            vel = vel_before_last
        t += n_in * dt if n_in > 1 else dt
        steps += 1
        taken += 1
        out = dict(pos=pos, vel=vel, rho=rho, p=p, drho_dt=drho_dt, force=force, force_prior=fp, Vol=Vol, B=B)
    if out is None:  # no step taken from a fresh start: the state as given, the outputs of a step at zero
        out = dict(pos=pos, vel=vel, rho=np.zeros(nt), p=np.zeros(nt), drho_dt=drho_dt, force=np.zeros((nt, 2), order="F"),
                   force_prior=np.zeros((nt, 2), order="F"), Vol=np.zeros(nt), B=np.zeros((nt, 4), order="F"))
    out.update(t=t, dt_last=dt, vmax=_vmax(out["vel"], nf), steps=steps)
    return out


# ---- the shared starts: 600 fluid particles, dp = 0.05, DL = 1.5, DH = 1 ----

def plain(cfgmod, geom, **kw):
    """The start of tests/test_gpu_load_chains.py: developed profile, positions jittered by 0.2 dp.  kw: other physics, as
    U_bulk < 0 of the start "left" (g, and with it the developed profile, point to the left)."""
    prm = cfgmod.params_from_values(dp=DP, DL=DL, **kw)
    parts = dict(geom.init_particles(prm))
    pos, vel = geom.developed_state(prm, parts, jitter=0.2, seed=21)
    assert parts["n_fluid"] == 600 and abs(prm.DH - 1.0) < 1e-12
    parts.update(pos=pos, vel=vel)
    return prm, parts


def squeezed(cfgmod, geom, centre, radius=4.5 * DP, factor=0.7):
    """plain() with the fluid within `radius` of `centre` drawn towards it to `factor` of its distance; the distance is taken
    with the minimum image in x and the result wrapped into [0, DL), so the centre may lie on the periodic seam."""
    prm, parts = plain(cfgmod, geom)
    nf = parts["n_fluid"]
    pos = parts["pos"]
    c = np.asarray(centre, dtype=np.float64)
    d = pos[:nf] - c
    d[:, 0] -= prm.DL * np.round(d[:, 0] / prm.DL)
    inside = np.hypot(d[:, 0], d[:, 1]) < radius
    new = c + factor * d[inside]
    x = new[:, 0] - np.floor(new[:, 0] / prm.DL) * prm.DL
    new[:, 0] = np.where(x >= prm.DL, x - prm.DL, x)  # (a tiny negative x rounds to DL)
    pos[:nf][inside] = new
    return prm, parts


def variant(cfgmod, geom):
    """Moving walls with a velocity per wall particle, uneven mass, rho0 = 2.5 (helpers.make_variant)."""
    from helpers import make_variant
    prm, parts = make_variant(cfgmod, geom, dp=DP, DL=DL, jitter=0.2, seed=31, developed=True, rho0=2.5, transport_coeff=0.1)
    assert parts["n_fluid"] == 600
    return prm, parts


def counts_within(prm, parts, radius):
    """Per fluid particle, by brute force with the minimum image in x: how many particles (fluid or wall) lie within `radius`,
    itself excluded; and how many of them are wall particles."""
    nf = parts["n_fluid"]
    p = np.asarray(parts["pos"])
    dx = p[:nf, None, 0] - p[None, :, 0]
    dx -= prm.DL * np.round(dx / prm.DL)
    dy = p[:nf, None, 1] - p[None, :, 1]
    r2 = dx * dx + dy * dy
    near = (r2 < radius * radius) & (r2 > 1e-24)
    return near.sum(axis=1), near[:, nf:].sum(axis=1)


def errors(got, ref):
    """max |a - b| / max |b| per field."""
    out = {}
    for k in FIELDS:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape and np.all(np.isfinite(a)), k
        out[k] = float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))
    return out


# The cases of tests/test_gpu_dual_rate_parity.py: name -> (start, lanes per particle, dual_rate = n_in, outer steps).  The CPU
# tests check every start's conditioning at these lengths, so a GPU case added here is covered by them.
GPU_CASES = {
    "A": ("plain", (32,), 2, 10),
    "B": ("plain", (16,), 2, 10),
    "C": ("plain", (16,), 3, 6),
    "D": ("plain", (32,), 4, 5),
    "E": ("bottom", (16,), 2, 6),
    "F": ("seam", (16,), 2, 6),
    "G": ("top", (16,), 3, 4),
    "H": ("variant", (16, 32), 2, 10),
    "I": ("plain", (16,), 2, 10),  # with rebuild_every = 4
    "J": ("plain", (16,), 2, 5),   # advance(2.5 Dt_first): 3 outer steps, then 2 more
    "K": ("bottom", (16,), 4, 3),  # max |v| > c_f / (n_in - 1): the advective limit sets Dt
    "L": ("left", (16,), 2, 10),   # U_bulk < 0: the flow, and the seam crossings, to the left
}


def start(cfgmod, geom, name):
    if name == "plain":
        return plain(cfgmod, geom)
    if name == "left":
        return plain(cfgmod, geom, U_bulk=-0.666667)
    if name == "variant":
        return variant(cfgmod, geom)
    return squeezed(cfgmod, geom, SQUEEZE_CENTRES[name])
