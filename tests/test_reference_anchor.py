"""The CPU oracle against the reference's own C code (not gpu).

oracle/Makefile builds the reference's two MEX files, unmodified, against the mocked MATLAB C API of tests/stubs (serial,
-O2 -ffp-contract=off: the oracle's flags) into oracle/_ref/.  oracle/sph_oracle.c restates the same arithmetic in the same
order, so the neighbour search and every physics mode must agree BIT FOR BIT, pair order included; a difference is a bug on
one side and gets no tolerance.  The time loop is driver.run(engine="mex") over the reference's binaries against oracle.run.
These tests skip only where there is neither a built oracle/_ref/ nor a reference checkout to build it from."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mex_mock
import pair_list_cases
import reference_ids_worker
import regime_cases
from helpers import make_case, make_variant, oracle_surface, run_modes

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "reference_small.npz")


@pytest.fixture(scope="module")
def ref(oracle):
    r = mex_mock.reference_mex()
    if r is None:
        pytest.skip("neither oracle/_ref/ nor a reference checkout (SPHX_REFERENCE_DIR) exists")
    return r


def _defects(cfgmod, geom):
    from test_gpu_edge_cases import _case_with_defects
    return _case_with_defects(cfgmod, geom)


def _outside(cfgmod, geom):
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=1.5, jitter=0.1, seed=5, developed=True)
    parts["pos"][5] = (0.4, 2.5)
    parts["vel"][5] = (0.0, 0.0)
    return prm, parts


CASES = {
    "lattice": lambda c, g: make_case(c, g, dp=0.05, DL=3.0, jitter=0.0, developed=False, seed=100),
    "dp004_jitter03": lambda c, g: make_case(c, g, dp=0.04, DL=3.0, jitter=0.3, seed=102),
    "dp0025_DL1": lambda c, g: make_case(c, g, dp=0.025, DL=1.0, jitter=0.25, seed=103),
    "dp005_DL07": lambda c, g: make_case(c, g, dp=0.05, DL=0.7, jitter=0.2, seed=104),
    "rho25": lambda c, g: make_case(c, g, dp=0.05, DL=1.5, seed=105, rho0=2.5, mu=0.07, c_f=12.0, U_bulk=0.4, transport_coeff=0.1),
    "DH08_rho037": lambda c, g: make_case(c, g, dp=0.04, DL=1.3, DH=0.8, seed=106, rho0=0.37, mu=0.2, c_f=20.0),
    "moving_walls": lambda c, g: make_variant(c, g, dp=0.05, DL=1.5, seed=107, rho0=2.5, transport_coeff=0.1),
    "moving_walls_DH08": lambda c, g: make_variant(c, g, dp=0.04, DL=1.3, DH=0.8, seed=108, rho0=0.37),
    "density_floor": lambda c, g: regime_cases.floor(c, g, "small"),
    "coincident_isolated": _defects,
    "outside_cell_rows": _outside,
    "two_columns_07": lambda c, g: make_case(c, g, dp=0.1, DL=0.7, jitter=0.25, seed=9),
    "two_columns_06": lambda c, g: make_case(c, g, dp=0.1, DL=0.6, jitter=0.25, seed=9),
    "one_column_04": lambda c, g: make_case(c, g, dp=0.1, DL=0.4, jitter=0.2, seed=4, developed=False),
    "one_column_02": lambda c, g: make_case(c, g, dp=0.1, DL=0.2, jitter=0.2, seed=4, developed=False),
    # the regimes of tests/regime_cases.py: leftward flow, capped Riemann dissipation, viscous-limited dt (its floor case is
    # density_floor above)
    "leftward": lambda c, g: regime_cases.leftward(c, g, "small"),
    "capped": lambda c, g: regime_cases.capped(c, g, "small"),
    "left_capped": lambda c, g: regime_cases.left_capped(c, g, "small"),
    "viscous": lambda c, g: regime_cases.viscous(c, g, "small"),
}


@pytest.fixture(scope="module", params=list(CASES))
def case(request, cfgmod, geom, oracle):
    prm, parts = CASES[request.param](cfgmod, geom)
    nb = oracle.neighbor_search(parts["pos"], parts["n_fluid"], parts["n_total"], prm.h, prm.DL)
    return prm, parts, nb


def same_bits(a, b, name):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, f"{name}: shape {a.shape} vs {b.shape}"
    bad = a.view(np.uint64) != b.view(np.uint64)
    assert not np.any(bad), (f"{name}: {int(bad.sum())}/{a.size} elements differ in their bits, max |a-b| "
                             f"{np.nanmax(np.abs(a - b)):.3e} at {np.argwhere(bad)[:3].tolist()}")


def check_modes(ref, oracle, prm, parts, nb, tag="", monitor=True, h=None):
    """The eight modes, chained as SPH_Poiseuille.m chains them, on one pair list: reference against oracle, bit for bit.
    h: what the modes take as h where it is not prm.h (a list built with a wider kernel)."""
    nf, nt = parts["n_fluid"], parts["n_total"]
    mass, pos, vel, wv, drho = (parts[k] for k in ("mass", "pos", "vel", "wall_vel", "drho_dt"))
    h = prm.h if h is None else h
    p6 = tuple(nb[:5]) + (nb[6],)
    phys = ref.sph_physics_shell_mex
    rho, Vol, B = oracle.density_correction(nb, mass, nf, nt, prm.rho0, h, prm.inv_sigma0)
    for g, r, n in zip(phys("density_correction", *nb, mass, nf, nt, prm.rho0, h, prm.inv_sigma0), (rho, Vol, B), ("rho", "Vol", "B")):
        same_bits(r, g, tag + "density." + n)
    fv = oracle.viscous_force(nb, vel, Vol, B, prm.mu, h, nf, nt, mass, wv)
    same_bits(fv, phys("viscous_force", *p6, vel, Vol, B, prm.mu, h, nf, nt, mass, wv), tag + "viscous(16)")
    same_bits(fv, phys("viscous_force", *p6, vel, Vol, B, prm.mu, h, nf, nt, mass, wv, 0.0), tag + "viscous(17)")
    same_bits(oracle.transport_correction(nb, Vol, B, pos, h, nf, nt, 0.2),
              phys("transport_correction", *p6, Vol, B, pos, h, nf, nt), tag + "transport()")
    for coeff in (0.3, prm.transport_coeff):
        same_bits(oracle.transport_correction(nb, Vol, B, pos, h, nf, nt, coeff),
                  phys("transport_correction", *p6, Vol, B, pos, h, nf, nt, coeff), tag + f"transport({coeff})")
    fp = fv.copy(order="F")
    fp[:nf, 0] += mass[:nf] * prm.gravity_g
    dt = 0.25 * prm.h / (prm.c_f + 1.0)
    common = (Vol, B, rho, mass, pos, vel, drho, fp, dt, nf, nt, prm.rho0, prm.p0, prm.c_f, wv)
    o1 = oracle.integration_1st(nb, *common)
    for g, r, n in zip(phys("integration_1st", *p6, *common), o1, ("rho", "p", "pos", "force", "drho")):
        same_bits(r, g, tag + "int1." + n)
    rho_h, p_h, pos_h, force1, _ = o1
    vel_new = vel.copy(order="F")
    vel_new[:nf] += (fp[:nf] + force1[:nf]) / mass[:nf, None] * dt
    for g, r, n in zip(phys("integration_2nd", *p6, Vol, rho_h, pos_h, vel_new, dt, nf, nt, wv),
                       oracle.integration_2nd(nb, Vol, rho_h, pos_h, vel_new, dt, nf, nt, wv), ("pos", "drho", "zeros")):
        same_bits(r, g, tag + "int2." + n)
    for g, r, n in zip(phys("integration_verlet", *p6, *common), oracle.integration_verlet(nb, *common),
                       ("rho", "p", "pos", "vel", "drho", "force")):
        same_bits(r, g, tag + "verlet." + n)
    tail = (mass, pos, vel, wv, rho, drho, dt, nf, nt, prm.rho0, prm.p0, prm.c_f, prm.mu, h, prm.inv_sigma0, prm.gravity_g)
    for g, r, n in zip(phys("advance_shell_step", *nb, *tail), oracle.advance_shell_step(nb, *tail),
                       ("rho", "p", "pos", "vel", "drho", "force", "force_prior", "Vol", "B")):
        same_bits(r, g, tag + "advance." + n)
    if monitor:
        check_monitor(ref, oracle, prm, parts, nb, Vol, B, tag, h)


def check_monitor(ref, oracle, prm, parts, nb, Vol, B, tag="", h=None):
    h = prm.h if h is None else h
    nf, pos, vel, wv = parts["n_fluid"], parts["pos"], parts["vel"], parts["wall_vel"]
    p6 = tuple(nb[:5]) + (nb[6],)
    phys = ref.sph_physics_shell_mex
    same_bits(np.array(oracle.wall_shear_monitor(nb, pos, vel, wv, Vol, B, nf, prm.DL, prm.DH, prm.mu, h)),
              np.array(phys("wall_shear_monitor", *p6, pos, vel, wv, Vol, B, nf, prm.DL, prm.DH, prm.mu, h)), tag + "tau")


def test_neighbor_search_is_bit_identical(case, ref):
    prm, parts, nb = case
    got = ref.sph_neighbor_search_mex(parts["pos"], parts["n_fluid"], parts["n_total"], prm.h, prm.DL)
    assert len(got[0]) == len(nb[0])
    for g, r, n in zip(got, nb, ("pair_i", "pair_j", "dx", "dy", "r", "W", "dW")):
        same_bits(r, g, n)


def test_modes_are_bit_identical(case, ref, oracle):
    prm, parts, nb = case
    check_modes(ref, oracle, prm, parts, nb)


def test_modes_on_an_empty_pair_list(ref, oracle, cfgmod, geom):
    prm, parts = make_variant(cfgmod, geom, dp=0.05, DL=1.0, jitter=0.1, seed=2, rho0=2.5)
    check_modes(ref, oracle, prm, parts, (np.zeros(0),) * 7)


def test_modes_skip_out_of_range_pair_indices_alike(ref, oracle, cfgmod, geom):
    """i = 0, i = a wall row, j = 0, j beyond n_total (the rows of test_gpu_edge_cases.py), plus j = n_total + 7 on a valid i.
    wall_shear_monitor sees only the first three: its guard (sph_physics_mex.c:1722, `jj < n_fluid`) has no upper bound, so
    with j > n_total the reference reads past its arrays and returns whatever lies there -- outside its contract, nothing to
    compare."""
    prm, parts = make_variant(cfgmod, geom, dp=0.05, DL=1.0, jitter=0.1, seed=3, rho0=2.5)
    nf, nt = parts["n_fluid"], parts["n_total"]
    nb = oracle.neighbor_search(parts["pos"], nf, nt, prm.h, prm.DL)
    bad = [np.concatenate([c, c[:5]]) for c in nb]
    bad[0][-5:] = [0, nf + 1, 1, 2, 3]
    bad[1][-5:] = [1, 2, 0, nt + 5, nt + 7]
    check_modes(ref, oracle, prm, parts, tuple(bad), monitor=False)
    rho, Vol, B = oracle.density_correction(nb, parts["mass"], nf, nt, prm.rho0, prm.h, prm.inv_sigma0)
    check_monitor(ref, oracle, prm, parts, tuple(c[:-2] for c in bad), Vol, B)
    good = oracle.density_correction(nb, parts["mass"], nf, nt, prm.rho0, prm.h, prm.inv_sigma0)
    for a, b in zip(oracle.density_correction(tuple(bad), parts["mass"], nf, nt, prm.rho0, prm.h, prm.inv_sigma0), good):
        same_bits(a, b, "bad rows ignored")


# ---- the pair lists of tests/pair_list_cases.py: any order, either side first, skipped, repeated, coincident, empty, long rows ----
PERMUTATION_BOUND = 1e-13  # helpers.assert_close's atol_scale; measured 6.3e-15 (int1.drho, moving_walls), 3.1e-15 on capped


@pytest.fixture(scope="module", params=list(pair_list_cases.STATES))  # the GPU tests' own states
def lists(request, cfgmod, geom, oracle):
    prm, parts = pair_list_cases.STATES[request.param](cfgmod, geom)
    nb = oracle.neighbor_search(parts["pos"], parts["n_fluid"], parts["n_total"], prm.h, prm.DL)
    return prm, parts, nb, pair_list_cases.contract_lists(oracle, prm, parts, nb)


@pytest.mark.parametrize("name", ["shuffled", "any_order", "one_sided", "skipped", "repeats", "coincident", "empty_rows", "wide"])
def test_modes_are_bit_identical_on_every_legal_list(name, lists, ref, oracle):
    """The reference walks any list front to back and so does the oracle: bit for bit on every list of pair_list_cases, which
    makes the oracle the judge of the HIP surface on them (tests/test_gpu_pair_list_contract.py).  wall_shear_monitor gets the
    skipped rows without j > n_total (see test_modes_skip_out_of_range_pair_indices_alike)."""
    prm, parts, _, all_lists = lists
    c = all_lists[name]
    check_modes(ref, oracle, prm, parts, c["nb"], tag=name + ": ", monitor=c["monitor_nb"] is None, h=c["h"])
    if c["monitor_nb"] is not None:
        nf, nt = parts["n_fluid"], parts["n_total"]
        _, Vol, B = oracle.density_correction(c["nb"], parts["mass"], nf, nt, prm.rho0, c["h"], prm.inv_sigma0)
        check_monitor(ref, oracle, prm, parts, c["monitor_nb"], Vol, B, name + ": ", c["h"])


def test_pair_lists_are_what_they_claim(lists, oracle, capsys):
    """A census of pair_list_cases over the oracle alone: half of the fluid-fluid rows swapped, the one-sided rows one-sided,
    the wide rows >= 100 entries long, repeats and coincident rows present and changing the answer, the skipped rows skipped
    EXACTLY (every oracle output bit for bit the clean list's) and the oracle order-invariant to round-off: a permutation plus
    the swap moves no output by more than PERMUTATION_BOUND of its field's largest magnitude (measured: 6.3e-15 at worst)."""
    prm, parts, nb, L = lists
    nf, nt = parts["n_fluid"], parts["n_total"]
    ff = pair_list_cases.fluid_fluid(nb, nf)
    wall_first = lambda l: np.any((l[0] > nf) & (l[0] <= nt) & (l[1] <= nf))
    # shuffled / swapped
    assert sorted(L["shuffled"]["perm"].tolist()) == list(range(len(nb[0]))) and np.any(np.diff(L["shuffled"]["nb"][0]) < 0)
    any_order = L["any_order"]["nb"]
    share = len(L["any_order"]["swapped_rows"]) / np.count_nonzero(ff)
    assert 0.4 <= share <= 0.6, share
    assert np.count_nonzero(pair_list_cases.fluid_fluid(any_order, nf) & (any_order[0] > any_order[1])) == len(L["any_order"]["swapped_rows"])
    assert not wall_first(any_order) and len(any_order[0]) == len(nb[0])
    # one-sided: rows that are purely second-side, and rows without a second side
    one = L["one_sided"]
    assert pair_list_cases.is_one_sided(one["nb"], nf, one["always_second"], one["always_first"])
    assert len(one["always_second"]) == len(one["always_first"]) == 5 and not wall_first(one["nb"])
    assert not np.any(np.isin(one["nb"][0][one["nb"][1] > nf].astype(int) - 1, one["always_second"]))
    # long rows
    wide_rows = pair_list_cases.row_lengths(L["wide"]["nb"], nf)
    assert wide_rows.min() >= 100 and 4 * L["wide"]["h"] <= prm.DL, (wide_rows.min(), wide_rows.max())
    assert pair_list_cases.row_lengths(nb, nf).max() <= 64
    # repeats, coincident, emptied rows
    assert L["repeats"]["mask"].sum() == 40 and len(L["repeats"]["nb"][0]) == len(nb[0]) + 40
    rep = np.column_stack(L["repeats"]["nb"])
    assert len(np.unique(rep, axis=0)) == len(nb[0])
    co, co_mask = L["coincident"]["nb"], L["coincident"]["mask"]
    assert co_mask.sum() == 3 and np.array_equal(np.flatnonzero(co[4] == 0.0), np.flatnonzero(co_mask))
    ci, cj = co[0][co_mask], co[1][co_mask]
    assert sorted([("ff<" if i < j <= nf else "ff>" if j < i else "fw") for i, j in zip(ci, cj)]) == ["ff<", "ff>", "fw"]
    assert np.all(pair_list_cases.row_lengths(L["empty_rows"]["nb"], nf)[L["empty_rows"]["emptied"]] == 0)
    assert set(L["empty_rows"]["emptied"].tolist()) >= {0, nf - 1} and len(L["empty_rows"]["emptied"]) == 4
    # skipped rows: every kind present, NaN geometry, and skipped exactly
    sk, mask = L["skipped"]["nb"], L["skipped"]["mask"]
    assert mask.sum() == 64 and all(np.all(np.isnan(c[mask])) for c in sk[2:]) and 0 < np.flatnonzero(mask)[0] and np.flatnonzero(mask)[-1] < len(mask) - 1
    assert all(np.array_equal(c[~mask], k) for c, k in zip(sk, any_order))
    bi, bj = sk[0][mask], sk[1][mask]
    for kind in (bi == 0, bi == nf + 1, bi == nt, bi == -3, bj == 0, bj == -1, bj == nt + 1, bj == nt + 5):
        assert np.count_nonzero(kind) >= 64 // 8
    mon, mon_mask = L["skipped"]["monitor_nb"], L["skipped"]["monitor_mask"]
    assert mon_mask.sum() == 64 and np.all(mon[1] <= nt) and np.all(np.isnan(mon[4][mon_mask]))
    phys = oracle_surface(oracle)
    clean = run_modes(phys, prm, parts, any_order)
    poisoned = run_modes(phys, prm, parts, sk, monitor_nb=mon)
    for k in clean:
        same_bits(poisoned[k], clean[k], "skipped rows: " + k)
    # the oracle on its own list against the shuffled and half-swapped one
    plain = run_modes(phys, prm, parts, nb)
    moved = {k: float(np.max(np.abs(np.asarray(clean[k]) - np.asarray(plain[k]))) / max(np.max(np.abs(plain[k])), 1e-300)) for k in plain}
    worst = max(moved, key=moved.get)
    with capsys.disabled():
        print(f"\n[pair lists] a permutation + swap moves the oracle by at most {moved[worst]:.1e} ({worst})")
    assert moved[worst] <= PERMUTATION_BOUND, moved
    # repeated and coincident rows count: a surface that dropped them could not match the oracle
    for name in ("repeats", "coincident"):
        rho = run_modes(phys, prm, parts, L[name]["nb"])
        assert all(np.all(np.isfinite(v)) for v in rho.values()), name
        assert np.max(np.abs(rho["density.rho"] - clean["density.rho"])) > 1e-3 * np.max(np.abs(clean["density.rho"])), name


LOOP_FIELDS = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B")
LOOP_BOUND = 1e-12
# Worst value seen over LOOP_CASES x (10, 35) steps.  Every step but the last is bit-identical; the last dt differs in its last
# bits (clipped to t_end - t against unclipped), which the stiff EOS turns into 9e-15 of p.  Vol, B and force_prior do not
# depend on the last dt, and t lands on t_end exactly: measured 0, so asserted bit-identical.
MEASURED_LOOP = dict(t=0.0, dt=9.7e-16, tau=2.9e-16, pos=1.5e-16, vel=2.0e-16, rho=3.4e-16, p=8.8e-15, drho_dt=8.0e-16,
                     force=3.8e-15, force_prior=0.0, Vol=0.0, B=0.0)


def loop_differences(driver, ref, oracle, cfgmod, prm_kw, parts, n_steps):
    """n_steps of oracle.run, then the driver's MEX loop over the reference's binaries to the time the oracle reached (that
    loop has no step limit, so its last dt is clipped by `remain` to land there).  -> worst difference per field, relative to
    the field's largest magnitude; t, dt and tau relative."""
    prm0 = cfgmod.params_from_values(**prm_kw)
    want = oracle.run(prm0, parts, t_end=1e9, output_interval=1e9, max_steps=n_steps, enable_sort=False)
    t_end = want["stats"]["t"]
    prm = cfgmod.params_from_values(end_time=t_end, output_interval=t_end, **prm_kw)
    res, got = mex_mock.run_driver_loop(driver, ref, prm, parts)
    diffs = {"t": abs(res.t - t_end) / t_end, "dt": abs(got["dt"] - want["stats"]["dt_last"]) / want["stats"]["dt_last"],
             "tau": max(abs(res.tau_bottom - want["stats"]["tau_bottom"]), abs(res.tau_top - want["stats"]["tau_top"]))
             / max(abs(want["stats"]["tau_bottom"]), abs(want["stats"]["tau_top"]))}
    for k in LOOP_FIELDS:
        a, b = np.asarray(got[k]).reshape(np.asarray(want[k]).shape), np.asarray(want[k])
        assert np.all(np.isfinite(a)), k
        diffs[k] = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    return res, want, got, diffs


LOOP_CASES = {
    "default": (False, dict(dp=0.05, DL=1.5, jitter=0.2, seed=7), {}),
    "moving_walls": (True, dict(dp=0.05, DL=1.5, jitter=0.2, seed=7), dict(rho0=2.5, mu=0.07, c_f=12.0, U_bulk=0.4, transport_coeff=0.1)),
    "leftward": (False, dict(dp=0.05, DL=1.5, jitter=0.2, seed=7), dict(U_bulk=-0.666667)),
    "capped": (False, dict(dp=0.05, DL=1.5, jitter=0.2, seed=7), dict(c_f=0.3)),
    "viscous": (False, dict(dp=0.05, DL=1.5, jitter=0.2, seed=7), dict(mu=2.0)),
}


@pytest.mark.parametrize("n_steps", [10, 35])
@pytest.mark.parametrize("name", list(LOOP_CASES))
def test_time_loop_over_the_reference_matches_oracle_run(name, n_steps, ref, oracle, driver, cfgmod, geom, capsys):
    """driver.run(engine="mex") with the reference's binaries in place of the HIP surface, against oracle.run, enable_sort
    off.  The dt rule on the reference's side is driver.verlet_time_step, so this ties the oracle's dt to the driver's.  Not
    bit-exact: oracle.run stops on a step count, the driver on t_end, so the driver's last dt is clipped to `remain`, which
    differs from the unclipped dt by round-off of t.  Measured worst difference per field, relative to the field's largest
    magnitude (t, dt, tau: relative), over both cases and both step counts: MEASURED_LOOP above, at most 9.7e-16 for dt,
    8.8e-15 for p, 3.8e-15 for force and below 1e-15 for every other field.  Asserted: ten times that, and never more than
    1e-12, the suite's tolerance for the dt sequence."""
    moving, kw, prm_kw = LOOP_CASES[name]
    make = make_variant if moving else make_case
    _, parts = make(cfgmod, geom, **kw, **prm_kw)
    prm_kw = dict(prm_kw, dp=kw["dp"], DL=kw["DL"])
    res, want, got, diffs = loop_differences(driver, ref, oracle, cfgmod, prm_kw, parts, n_steps)
    with capsys.disabled():
        print(f"\n[loop {name}@{n_steps}] " + " ".join(f"{k}={v:.2e}" for k, v in diffs.items()))
    assert res.steps == n_steps == want["stats"]["steps"]
    assert got["n_pairs"] == want["stats"]["n_pairs_last"]
    for k, v in diffs.items():
        assert v <= min(10 * MEASURED_LOOP[k], LOOP_BOUND), (k, v)



def test_error_identifiers_equal_the_references(mex, ref):
    """Every malformed call of reference_ids_worker.MALFORMED: the identifier of the reference's own mexErrMsgIdAndTxt (made
    in a child process, which a call that the reference does not reject could crash) equals the one mex_surface.py raises."""
    p = subprocess.run([sys.executable, os.path.join(HERE, "reference_ids_worker.py")], capture_output=True, text=True, timeout=120)
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0, f"the child ended with {p.returncode} after {lines[-1:]}: {p.stderr[-2000:]}"
    got = {l["k"]: l["id"] for l in lines if "id" in l}
    assert len(got) == len(reference_ids_worker.MALFORMED)
    for k, (fn, nargout, args) in enumerate(reference_ids_worker.MALFORMED):
        want = reference_ids_worker.call(mex, fn, nargout, args)
        assert want is not None and got[k] == want, (k, fn, args[:1], got[k], want)
