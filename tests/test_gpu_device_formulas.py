"""The device formulas one by one (gpu): every floating-point __device__ function of csrc/sphx_device.hpp, and the geometry and
clock helpers of csrc/sphx_kernels.hpp, called alone through the harness library (tests/devtest.py) and compared with the exact
references of tests/device_cases.py on its hand-placed inputs.

Bounds (eps = 2^-52):
  rcp_nr, rsqrt_nr     relative error <= 2 eps (the header promises about 1; a correctly rounded 1 / sqrt measures 0.75)
  pair_geom            r within 3 eps of sqrt(dx^2 + dy^2) (device_cases.PAIR_GEOM_R_BOUND), |ex^2 + ey^2 - 1| <= 4 eps
  spline forms, pair terms, the small rational formulas
                       |device - exact| <= 2 x (worst |numpy double - exact| of the same form over the same inputs) + 2 eps of
                       the function's scale (sigma for W, sigma / h for dW, the largest product for a pair term)
  kgc_from_A           4 x numpy double's own error + 1e-15
  riemann_beta, min_image   bit-exact against numpy
Each test prints `function: worst error ... (allowed ...)`; the figures of an MI355X are in profiles/r33_device_formulas.txt."""
import numpy as np
import pytest

import device_cases as dc
import devtest

pytestmark = pytest.mark.gpu
na = np.nextafter
EPS = dc.EPS


def report(name, worst, allowed, unit="eps"):
    print("%s: worst error %.3g %s (allowed %.3g)" % (name, worst, unit, allowed))


# ---- A. per-pair arithmetic ----
def test_rcp_nr_is_within_two_ulp():
    x = dc.rcp_inputs()
    (y,), _ = devtest.call("F_RCP_NR", [x])
    err = np.abs(dc.rcp_rel_error(x, y))
    report("rcp_nr", err.max(), 2.0)
    (o,), _ = devtest.call("F_RCP_NR", [dc.OUT_OF_DOMAIN])
    print("rcp_nr outside its domain (not asserted):", dict(zip(dc.OUT_OF_DOMAIN.tolist(), o.tolist())))
    assert np.all(np.isfinite(y)) and err.max() <= 2.0, x[np.argmax(err)]
    assert np.all(y[np.log2(x) % 1 == 0] == 1.0 / x[np.log2(x) % 1 == 0])  # powers of two: exact


def test_rsqrt_nr_is_within_two_ulp():
    x = dc.rsqrt_inputs()
    (y,), _ = devtest.call("F_RSQRT_NR", [x])
    assert np.all(np.isfinite(y)) and np.all(y > 0)
    err = np.abs(dc.rsqrt_rel_error(x, y))
    base = np.abs(dc.rsqrt_rel_error(x, dc.np_rsqrt(x))).max()
    report("rsqrt_nr", err.max(), 2.0)
    print("rsqrt_nr: numpy 1.0 / sqrt(x) on the same inputs %.3g eps" % base)
    (o,), _ = devtest.call("F_RSQRT_NR", [dc.OUT_OF_DOMAIN])
    print("rsqrt_nr outside its domain (not asserted):", dict(zip(dc.OUT_OF_DOMAIN.tolist(), o.tolist())))
    assert err.max() <= 2.0, x[np.argmax(err)]


def test_pair_geom_distance_and_unit_vector():
    dx, dy = dc.pair_geom_inputs()
    (r, ex, ey), _ = devtest.call("F_PAIR_GEOM", [dx, dy])
    exact = dc.exact_r(dx, dy)
    err = dc.mp_rel_err(r, exact) / EPS
    report("pair_geom r", err.max(), dc.PAIR_GEOM_R_BOUND)
    unit = np.abs(dc.unit_defect(ex, ey))
    report("pair_geom ex^2 + ey^2 - 1", unit.max(), dc.PAIR_GEOM_UNIT_BOUND)
    assert err.max() <= dc.PAIR_GEOM_R_BOUND, (dx[np.argmax(err)], dy[np.argmax(err)])
    assert unit.max() <= dc.PAIR_GEOM_UNIT_BOUND
    # the unit vector points along (dx, dy): exact zeros and signs survive
    assert np.all(ex[dx == 0] == 0) and np.all(ey[dy == 0] == 0) and np.all(np.sign(ex) == np.sign(dx)) and np.all(np.sign(ey) == np.sign(dy))
    axis = dy == 0
    assert np.all(np.abs(np.abs(ex[axis]) - 1.0) <= 3 * EPS)


OP_OF_FORM = dict(spline="F_SPLINE", spline_dW="F_SPLINE_DW", spline_W="F_SPLINE_W", spline_dW_sel="F_SPLINE_DW_SEL",
                  spline_dW_in="F_SPLINE_DW_IN", spline_W_sel="F_SPLINE_W_SEL")


def spline_device(c, form, r=None):
    do, _ = devtest.call(OP_OF_FORM[form], [c["r"] if r is None else r], dpar=c["kc"])
    if form == "spline":
        return do[0], do[1]
    return (do[0], None) if form in ("spline_W", "spline_W_sel") else (None, do[0])


@pytest.mark.parametrize("dp", dc.DP_BASELINE)
@pytest.mark.parametrize("form", dc.SPLINE_FORMS)
def test_spline_form_against_the_exact_polynomial(form, dp):
    c, ref = dc.spline_inputs(dp), dc.spline_reference(dp)
    kc = c["kc"]
    got = spline_device(c, form)
    for which, exact, scale, g, np_err in (("W", ref["W"], kc[2], got[0], ref["np_err"][form][0]), ("dW", ref["dW"], kc[3], got[1], ref["np_err"][form][1])):
        if g is None:
            continue
        err = dc.frac_err(g, exact) / (EPS * scale)
        allowed = dc.spline_bound(np_err.max())
        report("%s %s dp=%g" % (form, which, dp), err.max(), allowed, "eps of scale (numpy double %.3g)" % np_err.max())
        assert err.max() <= allowed, c["r"][np.argmax(err)] / c["h"]


@pytest.mark.parametrize("dp", dc.DP_BASELINE)
def test_spline_forms_agree_on_both_sides_of_q_1(dp):
    c, ref = dc.spline_inputs(dp), dc.spline_reference(dp)
    m = c["near1"]
    out = {f: spline_device(c, f) for f in dc.SPLINE_FORMS}
    worst = 0.0
    for k, (scale, forms) in enumerate(((c["kc"][2], ("spline", "spline_W", "spline_W_sel")), (c["kc"][3], ("spline", "spline_dW", "spline_dW_sel", "spline_dW_in")))):
        for a in forms:
            for b in forms:
                if a < b:
                    diff = np.abs(out[a][k][m] - out[b][k][m]).max() / (EPS * scale)
                    allowed = dc.spline_bound(max(ref["np_err"][a][k].max(), ref["np_err"][b][k].max()))
                    worst = max(worst, diff / allowed)
                    assert diff <= allowed, (a, b, diff, allowed)
    report("spline forms around q = 1, dp=%g" % dp, worst, 1.0, "of the allowed difference")
    # the twins are one expression
    assert np.array_equal(out["spline"][0], out["spline_W"][0]) and np.array_equal(out["spline"][1], out["spline_dW"][1])


@pytest.mark.parametrize("dp", dc.DP_BASELINE)
def test_spline_preconditions(dp):
    c = dc.spline_inputs(dp)
    kc = c["kc"]
    # spline_dW_sel is clamped: zero (of either sign) from q = 2 on -- q the exact product r * inv_h, see device_cases.outside_q
    r_out = dc.outside_q(dp)
    _, dW = spline_device(c, "spline_dW_sel", r_out)
    assert np.all(dW == 0.0), dW
    for form in ("spline", "spline_dW", "spline_W"):
        W, dW2 = spline_device(c, form, r_out)
        assert (W is None or np.all(W == 0.0)) and (dW2 is None or np.all(dW2 == 0.0))
    # spline_dW_in / spline_W_sel are not: just beyond 2 h they leave a rounding error's worth, below 1e-28 of their scale
    r_b = dc.beyond_support(dp)
    _, dW = spline_device(c, "spline_dW_in", r_b)
    W, _ = spline_device(c, "spline_W_sel", r_b)
    report("spline_dW_in just beyond 2h, dp=%g" % dp, np.abs(dW).max() / kc[3], 1e-28, "of sigma/h")
    report("spline_W_sel just beyond 2h, dp=%g" % dp, np.abs(W).max() / kc[2], 1e-28, "of sigma")
    assert np.abs(dW).max() < 1e-28 * kc[3] and np.abs(W).max() < 1e-28 * kc[2]


@pytest.mark.parametrize("term", ("kgc_moment_add", "continuity_add", "wall_pair", "wall_pressure_add"))
def test_pair_term_of_one_pair(term):
    c, ref = dc.pair_term_inputs(), dc.pair_term_reference()[term]
    do, _ = devtest.call("F_" + term.upper(), [c[k] for k in ref["cols"]], dpar=c["kc"])
    got = np.stack(do, 1)
    err = dc.mp_err(got, ref["exact"]) / (EPS * ref["scale"])
    for j in range(err.shape[1]):
        allowed = dc.rel_bound_rule(ref["np_err"][:, j].max())
        report("%s[%d]" % (term, j), err[:, j].max(), allowed, "eps of scale (numpy double %.3g)" % ref["np_err"][:, j].max())
        assert err[:, j].max() <= allowed, int(np.argmax(err[:, j]))
    if term == "continuity_add":  # a separating pair raises the density rate's sign opposite to an approaching one
        assert got[0, 0] * got[1, 0] < 0
    if term == "wall_pressure_add":  # face <= 0: the wall mirrors the particle's pressure, nothing added
        assert np.isfinite(got).all()


def test_kgc_from_A():
    k = dc.kgc_cases()
    do, _ = devtest.call("F_KGC_FROM_A", list(k["A"].T))
    B = np.stack(do, 1)
    err = dc.kgc_err(B, k["exact"], k["scale"])
    for g, name in ((0, "named and random"), (1, "rank one")):
        m = k["group"] == g
        allowed = dc.kgc_bound(k["np_err"][m].max())
        report("kgc_from_A, " + name, err[m].max(), allowed, "of max(1, |B|) (numpy double %.3g)" % k["np_err"][m].max())
        assert err[m].max() <= allowed, k["A"][m][np.argmax(err[m])]
    zero = k["names"].index("zero")
    assert B[zero].tolist() == [1.0, 0.0, 0.0, 1.0]  # B = I exactly


def test_riemann_beta_is_bit_exact():
    ul, ur, cf = dc.riemann_inputs()
    (b,), _ = devtest.call("F_RIEMANN_BETA", [ul, ur, cf])
    ref = dc.riemann_numpy(ul, ur, cf)
    wrong = dc.bits(b) != dc.bits(ref)
    report("riemann_beta", float(wrong.sum()), 0.0, "values differing in some bit")
    assert not wrong.any(), (ul[wrong][:3], ur[wrong][:3], b[wrong][:3], ref[wrong][:3])


def _rule_check(name, got, exact, np_val, scale):
    err = dc.frac_err(got, exact) / (EPS * scale)
    np_err = dc.frac_err(np_val, exact) / (EPS * scale)
    allowed = dc.rel_bound_rule(np_err.max())
    report(name, err.max(), allowed, "eps of scale (numpy double %.3g)" % np_err.max())
    assert err.max() <= allowed, int(np.argmax(err))


def test_transport_shift():
    t = dc.transport_cases()
    (sx, sy), _ = devtest.call("F_TRANSPORT_SHIFT", [t["inc_x"], t["inc_y"], t["h"], t["coeff"]])
    scale = t["coeff"] * t["h"] * t["h"] * np.maximum(np.hypot(t["inc_x"], t["inc_y"]), 1e-300)
    _rule_check("transport_shift x", sx, [e[0] for e in t["exact"]], t["np"][:, 0], scale)
    _rule_check("transport_shift y", sy, [e[1] for e in t["exact"]], t["np"][:, 1], scale)
    zero = (t["inc_x"] == 0) & (t["inc_y"] == 0)
    assert np.all(sx[zero] == 0) and np.all(sy[zero] == 0)
    # fade exactly 1: gain * inc and nothing else
    one = np.array([f == 1 for f in t["fade_exact"]]) & ~zero
    assert np.all(np.abs(sx[one] - t["np"][one, 0]) <= 2 * EPS * scale[one])


def test_density_from_sigma():
    d = dc.density_cases()
    (rho,), _ = devtest.call("F_DENSITY_FROM_SIGMA", d["cols"])
    n = d["n_random"]
    _rule_check("density_from_sigma", rho[:n], d["exact"][:n], d["np"][:n], np.abs(d["np"][:n]))
    # the hand-placed sums are exact in double: the floor at 1e-12 (<=) decides, to the bit
    assert np.array_equal(rho[n:], np.array([float(e) for e in d["exact"][n:]])), (rho[n:], d["exact"][n:])
    assert np.all(rho[n:][d["floored"][n:]] == d["cols"][3][n:][d["floored"][n:]])


def test_half_state():
    s = dc.half_state_cases()
    (rhoh, ph), _ = devtest.call("F_HALF_STATE", s["cols"])
    rho0, p0 = s["cols"][3], s["cols"][4]
    _rule_check("half_state rho", rhoh, [e[0] for e in s["exact"]], s["np"][:, 0], np.abs(s["np"][:, 0]))
    _rule_check("half_state p", ph, [e[1] for e in s["exact"]], s["np"][:, 1], p0 * np.maximum(np.abs(s["np"][:, 0]) / rho0, 1.0))
    assert np.all(rhoh[s["floored"]] == rho0[s["floored"]]) and np.all(ph[s["floored"]] == 0.0)
    assert np.all(rhoh[~s["floored"]] >= 1e-10)


def test_eos_pressure():
    e = dc.eos_cases()
    (p,), _ = devtest.call("F_EOS_PRESSURE", e["cols"])
    rho, rho0, p0 = e["cols"]
    _rule_check("eos_pressure", p, e["exact"], e["np"], p0 * np.maximum(rho / rho0, 1.0))
    assert np.all(p[rho == rho0] == 0.0) and np.sum(rho == rho0) == 2


# ---- B. geometry and the clock ----
@pytest.mark.parametrize("DL", dc.DL_CASES)
def test_wrap_x(DL):
    w = dc.wrap_cases(DL)
    (xw,), _ = devtest.call("G_WRAP_X", [w["x"], DL])
    err = dc.frac_err(xw, w["exact"]) / dc.ulp(DL)
    report("wrap_x DL=%g" % DL, err.max(), 1.0, "ulp(DL)")
    assert np.all(xw >= 0.0) and np.all(xw <= DL) and err.max() <= 1.0
    # DL itself comes back for the tiny negative x only (x + DL rounds to DL): -1e-17, -1e-300, -ulp(DL) / 4
    assert set(w["x"][xw == DL]) == {-1e-17, -1e-300, -dc.ulp(DL) / 4}
    assert np.all(xw[w["x"] == DL] == 0.0) and np.all(xw[w["x"] == -DL] == 0.0)


@pytest.mark.parametrize("which", range(len(dc.GRIDS)))
def test_cell_of(which):
    c = dc.cell_cases(which)
    _, (cx, cy) = devtest.call("G_CELL_OF", [c["x"], c["y"]], dpar=c["dpar"], ipar=[c["ncx"], c["ncy"], 0])
    assert cx.min() >= 0 and cx.max() < c["ncx"] and cy.min() >= 0 and cy.max() < c["ncy"]
    assert np.all(np.diff(cx) >= 0) and np.all(np.diff(cy) >= 0)  # x and y are sorted
    for got, exact, dist, length, name in ((cx, c["cx"], c["edge_dist_x"], c["DL"], "x"), (cy, c["cy"], c["edge_dist_y"], c["DH"], "y")):
        off = got != exact
        report("cell_of %s %s" % (c["name"], name), float(np.abs(got - exact).max()), 1.0, "columns, at %d of %d inputs" % (off.sum(), off.size))
        assert np.abs(got - exact).max() <= 1 and np.all(dist[off] <= 2 * dc.ulp(length))


@pytest.mark.parametrize("DL", dc.DL_CASES)
def test_cell_of_wrapped_x(DL):
    w = dc.wrap_cases(DL)
    ncx, ncy = 11, 3
    dpar = (0.0, 0.0, ncx / DL, ncy / 1.0, DL)
    y = np.full(w["x"].size, 0.5)
    _, (cx, _) = devtest.call("G_CELL_OF", [w["x"], y], dpar=dpar, ipar=[ncx, ncy, 1])
    (xw,), _ = devtest.call("G_WRAP_X", [w["x"], DL])
    _, (cx2, _) = devtest.call("G_CELL_OF", [xw, y], dpar=dpar, ipar=[ncx, ncy, 0])
    assert np.array_equal(cx, cx2) and cx.min() >= 0 and cx.max() < ncx
    assert np.all(cx[w["x"] == DL] == 0) and np.all(cx[w["x"] == -1e-17] == ncx - 1) and np.all(cx[w["x"] == na(DL, 0.0)] == ncx - 1)
    report("cell_of(wrap_x) DL=%g" % DL, 0.0, 0.0, "columns outside the grid")


@pytest.mark.parametrize("DL", dc.DL_CASES)
def test_min_image_is_bit_exact(DL):
    dx = dc.min_image_inputs(DL)
    half = 0.5 * DL
    (got,), _ = devtest.call("G_MIN_IMAGE", [dx], dpar=[DL, half])
    ref = dc.min_image_numpy(dx, DL, half)
    wrong = dc.bits(got) != dc.bits(ref)
    report("min_image DL=%g" % DL, float(wrong.sum()), 0.0, "values differing in some bit")
    assert not wrong.any()
    assert got[dx == half] == half and got[dx == -half] == -half                       # +-DL/2 does not fold
    assert got[dx == na(half, DL)] < 0 and got[dx == na(-half, -DL)] > 0              # the next double does
    (open_,), _ = devtest.call("G_MIN_IMAGE", [dx], dpar=[DL, np.inf])
    assert np.array_equal(dc.bits(open_), dc.bits(dx))                                 # an open window never folds


def test_neighbour_column_and_duplicate_column():
    cols = dc.column_cases()
    _, (ok, col, dup) = devtest.call("G_NEIGHBOUR_COLUMN", i=list(cols))
    seen = {}
    for (ncx, cx, ox, per), o, c, d in zip(cols.T.tolist(), ok, col, dup):
        assert d == int((ncx == 1 and ox != 0) or (ncx == 2 and ox == 1))
        if o:
            seen.setdefault((ncx, cx, per), []).append(int(c))
    keys = {(ncx, cx, per) for ncx, cx, ox, per in cols.T.tolist()}
    for key in keys:
        assert sorted(seen.get(key, [])) == dc.expected_columns(*key), key  # every distinct column, each once
    report("neighbour_column", 0.0, 0.0, "wrong sets over %d grids x columns" % len(keys))


def test_rebin_near():
    rows, exp = dc.rebin_cases()
    _, (near,) = devtest.call("G_REBIN_NEAR", i=list(rows))
    report("rebin_near", float((near != exp).sum()), 0.0, "wrong of %d" % exp.size)
    assert np.array_equal(near, exp)


def test_owns_by_position_and_by_column():
    lo, hi = 0.75, 1.5
    x = np.array([lo, na(lo, 0.0), na(lo, 1.0), hi, na(hi, 0.0), na(hi, 2.0), 0.0, 1.0, 2.0, -1.0])
    _, (own,) = devtest.call("G_OWNS", [x], [np.zeros(x.size)], dpar=[lo, hi], ipar=[0, 4, 0, 0])
    assert own.tolist() == ((x >= lo) & (x < hi)).astype(int).tolist()
    ncy, c0, c1 = 4, 2, 5
    cell = np.arange(7 * ncy)
    _, (own,) = devtest.call("G_OWNS", [np.full(cell.size, 99.0)], [cell], dpar=[lo, hi], ipar=[1, ncy, c0, c1])
    assert own.tolist() == ((cell // ncy >= c0) & (cell // ncy < c1)).astype(int).tolist()
    report("owns", 0.0, 0.0, "wrong")


def test_tracked_drift2():
    DL, half = 3.0, 1.5
    #            xo     yo     pbx    pby    cell
    rows = [(0.30, 0.50, 0.25, 0.45, 0), (0.01, 0.50, 2.99, 0.50, 0), (2.99, 0.50, 0.01, 0.50, 1), (np.nan, 0.5, 0.2, 0.5, 2), (0.3, np.nan, 0.2, 0.5, 2),
            (0.30, 0.50, 0.25, 0.45, 9), (np.nan, 0.5, 0.2, 0.5, 9), (1.0, 0.25, 1.0, 0.25, 3)]
    xo, yo, bx, by, cell = (np.array(v) for v in zip(*rows))
    (d2,), _ = devtest.call("G_TRACKED_DRIFT2", [xo, yo, bx, by], [cell], dpar=[DL, half], ipar=[0, 2, 0, 0])
    ddx = dc.min_image_numpy(xo - bx, DL, half)
    ref = ddx * ddx + (yo - by) ** 2
    assert d2[3] == np.inf and d2[4] == np.inf and d2[6] == np.inf and d2[7] == 0.0  # a NaN position: +inf
    ok = np.isfinite(ref)
    assert np.all(np.abs(d2[ok] - ref[ok]) <= 2 * EPS * ref[ok])
    assert abs(d2[1] - 0.02 ** 2) < 1e-15 and abs(d2[2] - 0.02 ** 2) < 1e-15               # across the seam: folded
    # a slab that owns by column (columns 0 .. 3 of ncy = 2 rows: cells 0 .. 7): cell 9 is not its own -> 0, NaN or not
    (d2s,), _ = devtest.call("G_TRACKED_DRIFT2", [xo, yo, bx, by], [cell], dpar=[DL, np.inf], ipar=[1, 2, 0, 4])
    assert d2s[5] == 0.0 and d2s[6] == 0.0 and d2s[3] == np.inf and d2s[0] == d2[0]
    assert abs(d2s[1] - 2.98 ** 2) < 1e-12                                               # an open window does not fold
    report("tracked_drift2", float(np.abs(d2[ok] - ref[ok]).max()), 2 * EPS * ref[ok].max(), "absolute")


def test_next_dt():
    names = list(dc.NEXT_DT_CASES)
    cols = [np.array([dc.NEXT_DT_CASES[k][j] for k in names] * 2) for j in range(8)]
    n_in = np.array([1] * len(names) + [3] * len(names))
    (dt,), _ = devtest.call("G_NEXT_DT", cols, [n_in])
    ref = dc.next_dt_numpy(*cols, n_in)
    err = np.abs(dt - ref) / np.spacing(ref)
    report("next_dt", err.max(), 1.0, "ulp")
    assert err.max() <= 1.0, dict(zip(names * 2, zip(dt, ref)))
    k = names.index("floor_remain_zero")
    assert dt[k] == 1e-12 and dt[names.index("floor_remain_negative")] == 1e-12 and dt[len(names) + k] == 1e-12
    assert dt[names.index("viscous")] == dc.NEXT_DT_CASES["viscous"][6] and dt[names.index("body")] == dc.NEXT_DT_CASES["body"][7]


def test_loop_continues():
    tt = 5.0
    edge = tt - 1e-12  # as the device computes it
    t = np.array([na(edge, 0.0), edge, na(edge, 9.0), 0.0, 0.0, 0.0, 0.0, 0.0, tt])
    steps = np.array([-1, -1, -1, 0, -1, 5, 5, 5, 5])
    status = np.array([0, 0, 0, 0, 0, 0, -4, 0, 0])
    rebuild = np.array([0, 0, 0, 0, 0, 0, 0, 1, 0])
    _, (go,) = devtest.call("G_LOOP_CONTINUES", [t, np.full(t.size, tt)], [steps, status, rebuild])
    assert go.tolist() == [1, 0, 0, 0, 1, 1, 0, 0, 0]
    report("loop_continues", 0.0, 0.0, "wrong")
