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


# ---- the eight modes of the stateless surface on one pair list ----
def oracle_surface(oracle):
    """oracle/oracle.py behind the call form of mex_surface.sph_physics_shell_mex(mode, pair columns..., arguments...)."""
    def phys(mode, *a):
        if mode in ("density_correction", "advance_shell_step"):
            return getattr(oracle, mode)(tuple(a[:7]), *a[7:])
        return getattr(oracle, mode)(tuple(a[:5]) + (a[5], a[5]), *a[6:])  # no W column: the six-column modes do not read it
    return phys


def modes_dt(prm):
    return 0.25 * prm.h / (prm.c_f + 1.0)


def run_modes(phys, prm, parts, nb, h=None, given=None, monitor_nb=None):
    """The eight modes on the pair list nb, chained as test_reference_anchor.check_modes chains them: density, viscous,
    transport (12 arguments, then with a coefficient), integration_1st, integration_2nd on the kicked velocity,
    integration_verlet, advance_shell_step, wall_shear_monitor.  -> {name: output}.  Every mode takes the outputs of the modes
    before it from `given` (the dict of an earlier run, the oracle's say, so that two sides are compared mode by mode on
    identical inputs) or, without one, from this run.  h replaces prm.h wherever a mode takes h (a list built with a wider
    kernel); monitor_nb is the list wall_shear_monitor gets where it is not nb."""
    nf, nt = parts["n_fluid"], parts["n_total"]
    mass, pos, vel, wv, drho = (parts[k] for k in ("mass", "pos", "vel", "wall_vel", "drho_dt"))
    h = prm.h if h is None else h
    nb = tuple(nb)
    p6 = nb[:5] + (nb[6],)
    out = {}

    def put(prefix, names, values):
        for n, v in zip(names, values):
            out[prefix + n] = v

    def src(name):
        return (out if given is None else given)[name]

    put("density.", ("rho", "Vol", "B"), phys("density_correction", *nb, mass, nf, nt, prm.rho0, h, prm.inv_sigma0))
    rho, Vol, B = src("density.rho"), src("density.Vol"), src("density.B")
    out["viscous"] = phys("viscous_force", *p6, vel, Vol, B, prm.mu, h, nf, nt, mass, wv)
    out["transport()"] = phys("transport_correction", *p6, Vol, B, pos, h, nf, nt)
    for coeff in (0.3, prm.transport_coeff):
        out[f"transport({coeff})"] = phys("transport_correction", *p6, Vol, B, pos, h, nf, nt, coeff)
    fp = np.array(src("viscous"), order="F")
    fp[:nf, 0] += mass[:nf] * prm.gravity_g
    dt = modes_dt(prm)
    common = (Vol, B, rho, mass, pos, vel, drho, fp, dt, nf, nt, prm.rho0, prm.p0, prm.c_f, wv)
    put("int1.", ("rho", "p", "pos", "force", "drho"), phys("integration_1st", *p6, *common))
    vel_new = vel.copy(order="F")
    vel_new[:nf] += (fp[:nf] + src("int1.force")[:nf]) / mass[:nf, None] * dt
    put("int2.", ("pos", "drho", "zeros"),
        phys("integration_2nd", *p6, Vol, src("int1.rho"), src("int1.pos"), vel_new, dt, nf, nt, wv))
    put("verlet.", ("rho", "p", "pos", "vel", "drho", "force"), phys("integration_verlet", *p6, *common))
    tail = (mass, pos, vel, wv, rho, drho, dt, nf, nt, prm.rho0, prm.p0, prm.c_f, prm.mu, h, prm.inv_sigma0, prm.gravity_g)
    put("advance.", ("rho", "p", "pos", "vel", "drho", "force", "force_prior", "Vol", "B"),
        phys("advance_shell_step", *nb, *tail))
    m = nb if monitor_nb is None else tuple(monitor_nb)
    out["tau"] = np.array(phys("wall_shear_monitor", *m[:5], m[6], pos, vel, wv, Vol, B, nf, prm.DL, prm.DH, prm.mu, h))
    return out


# ---- what several GPU test files share ----
HISTORY_FIELDS = ("step", "t", "dt", "vmax", "tau_bottom", "tau_top", "kinetic_energy", "u_bulk")
STATS_FIELDS = ("count", "sum_ux", "sum_ux2", "sum_uy", "sum_uy2")


def batch_members(cfgmod, geom, dp, DL, variants, jitter=0.2):
    """One (prm, parts) per variant (mu, c_f, transport_coeff, seed): capi.Batch.from_parts(*zip(*members)) is their batch."""
    return [make_case(cfgmod, geom, dp=dp, DL=DL, jitter=jitter, seed=v["seed"], developed=True, mu=v["mu"], c_f=v["c_f"],
                      transport_coeff=v["transport_coeff"]) for v in variants]


def full_state(dl, st, mon):
    """Everything a context or a batch member can be asked for after a step: download(), the status, monitor()."""
    return dict(dl, t=st["t"], dt_last=st["dt_last"], step=st["step"], vmax=st["vmax"], tau=np.array(mon[:2]),
                pairs=mon[2])


def stats_bands(prm):
    hw = max(prm.dp, prm.h)
    return [(0.5 * prm.DL, hw), (0.0, hw)]  # mid-channel and the periodic seam


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


def err_id(capi, fn, *args):
    """(error id, status) of a C ABI call that must be refused."""
    rc = fn(*args)
    assert rc != capi.SPHX_OK
    return capi.lib().sphx_last_error_id().decode(), rc


def gateway_cfg(prm, t_end):
    return dict(DL=prm.DL, DH=prm.DH, dp=prm.dp, h=prm.h, rho0=prm.rho0, mu=prm.mu, c_f=prm.c_f, p0=prm.p0,
                inv_sigma0=prm.inv_sigma0, gravity_g=prm.gravity_g, transport_coeff=prm.transport_coeff,
                t_end=t_end, sort_interval=prm.sort_interval)


def profiled_launches(ctx, n):
    ctx.profile_enable(True)
    ctx.advance(1e9, max_steps=n)
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    return {k: v["launches"] for k, v in prof.items() if v["launches"] > 0}  # (names seen earlier stay listed with 0)


def check_kernel_form(ctx, name):
    """The case `name` of a sampler test's CASES table runs the form of the step it is named after."""
    if name == "dp025_walk":
        assert ctx.kernel_forms()["walk_kernels"]
    if name == "dp05_dynamic":
        assert ctx.schedule()["dynamic"]
    if name == "dp025_dual":
        assert ctx.substeps() > 1
    if name.startswith("two_cols"):
        assert ctx.info()["n_cell_x"] == 2
    if name == "one_col":
        assert ctx.info()["n_cell_x"] == 1


def assert_sums_identical(a, b, what, fields=STATS_FIELDS):
    """Two lists of a sampler's raw sums, one dict per band: every array bit for bit, the same window."""
    for band, (x, y) in enumerate(zip(a, b)):
        for k in fields:
            assert np.array_equal(x[k], y[k]), f"{what}: band {band} {k}"
        assert (x["n_samples"], x["t_first"], x["t_last"]) == (y["n_samples"], y["t_first"], y["t_last"]), what


def oracle_history_rows(oracle, prm, parts, n_steps):
    """row k-1 = what the oracle's loop leaves after k steps (restarted from the initial state for every row)"""
    nf = parts["n_fluid"]
    rows = np.zeros((n_steps, 8))
    for k in range(1, n_steps + 1):
        ref = oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=k, enable_sort=False)
        s, v, m = ref["stats"], ref["vel"][:nf], ref["mass"][:nf]
        assert s["steps"] == k
        rows[k - 1] = (k, s["t"], s["dt_last"], s["vmax"], s["tau_bottom"], s["tau_top"],
                       np.sum(0.5 * m * (v[:, 0] ** 2 + v[:, 1] ** 2)), np.mean(v[:, 0]))
    return rows


def assert_history_matches_oracle(hist, want, what):
    n = len(want)
    assert list(hist["step"]) == list(range(1, n + 1)) and hist["n_dropped"] == 0, what
    got = {k: hist[k] for k in HISTORY_FIELDS}
    ref = {k: want[:, j] for j, k in enumerate(HISTORY_FIELDS)}
    tau_got = np.column_stack([got["tau_bottom"], got["tau_top"]])
    tau_ref = np.column_stack([ref["tau_bottom"], ref["tau_top"]])
    tau_scale = np.max(np.abs(tau_ref), axis=1, keepdims=True)
    print(f"{what}: max rel err t {rel_err(got['t'], ref['t']).max():.2e} dt {rel_err(got['dt'], ref['dt']).max():.2e} "
          f"vmax {rel_err(got['vmax'], ref['vmax']).max():.2e} tau (of the pair's larger) "
          f"{(np.abs(tau_got - tau_ref) / tau_scale).max():.2e} kinetic_energy "
          f"{rel_err(got['kinetic_energy'], ref['kinetic_energy']).max():.2e} u_bulk {rel_err(got['u_bulk'], ref['u_bulk']).max():.2e}")
    assert np.all(np.abs(got["t"] - ref["t"]) <= 1e-13 * ref["t"]), what
    assert np.all(np.abs(got["dt"] - ref["dt"]) <= 1e-12 * ref["dt"]), what
    assert np.all(np.abs(got["vmax"] - ref["vmax"]) <= 1e-9 * ref["vmax"]), what
    for k in range(n):  # the pair of one step together, as tests/test_gpu_resident.py compares monitor() with the oracle
        assert_close(tau_got[k], tau_ref[k], rtol=1e-8, atol_scale=1e-9, name=f"{what}: tau of step {k + 1}")
    assert np.all(rel_err(got["kinetic_energy"], ref["kinetic_energy"]) <= 1e-8), what
    assert np.all(rel_err(got["u_bulk"], ref["u_bulk"]) <= 1e-8), what
