"""The inputs and references of the device-function tests do what they are for (not gpu): conditions on tests/device_cases.py
itself, established with Fractions, mpmath and numpy alone, and on the harness library as a file -- never on what it computes.

Baseline (numpy double against exact, eps = 2^-52; spline_inputs of dp = 0.05, 0.025, 0.01, 0.002; seeds as committed):
  W, two-piece                       1.09 eps sigma      recorded bound 1.8
  dW, two-piece                      2.50 eps sigma/h    recorded bound 3.8
  W, branch-free without FMA         2.49 eps sigma      recorded bound 3.3
  dW, branch-free without FMA        3.14 eps sigma/h    recorded bound 3.6
  1.0 / sqrt(x)                      0.734 eps relative  recorded bound 0.75
asserted against the recorded bounds with a factor 1.25 of slack, so that another seed does not fail them.

Two guards of kgc_from_A cannot be entered by any finite input and have no case: |det N| < 1e-20 (N = A^T A + 1e-8 I has
det N >= 1e-16) and |det A + max(1 - det A, 0)| < 1e-12 (that sum is 1 up to rounding for det A <= 1, det A otherwise)."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import dense_cases
import device_cases as dc
import devtest

SLACK = 1.25
na = np.nextafter


# ---- baseline ----
@pytest.mark.parametrize("dp", dc.DP_BASELINE)
def test_numpy_double_splines_stay_within_the_recorded_baseline(dp):
    err = dc.spline_reference(dp)["np_err"]
    worst = dict(W_two_piece=max(err["spline"][0].max(), err["spline_W"][0].max()),
                 dW_two_piece=max(err["spline"][1].max(), err["spline_dW"][1].max()),
                 W_branch_free=err["spline_W_sel"][0].max(),
                 dW_branch_free=max(err["spline_dW_sel"][1].max(), err["spline_dW_in"][1].max()))
    print("dp %g: " % dp + ", ".join("%s %.2f (recorded %.1f)" % (k, v, dc.BASELINE[k]) for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= SLACK * dc.BASELINE[k], (k, v)
        assert v > 0.25, (k, v)  # (a reference that agrees with numpy to the bit would be numpy itself)


def test_numpy_reciprocal_square_root_stays_within_the_recorded_baseline():
    x = dc.rsqrt_inputs()
    worst = np.abs(dc.rsqrt_rel_error(x, dc.np_rsqrt(x))).max()
    print("1 / sqrt(x): %.3f eps (recorded %.2f)" % (worst, dc.BASELINE["rsqrt"]))
    assert 0.4 < worst <= SLACK * dc.BASELINE["rsqrt"]
    x = dc.rcp_inputs()
    assert np.abs(dc.rcp_rel_error(x, 1.0 / x)).max() <= 0.5  # a correctly rounded quotient


def test_numpy_double_small_formulas_are_close_to_exact():
    k = dc.kgc_cases()
    assert k["np_err"].max() < 1e-14
    t = dc.transport_cases()
    assert dc.frac_err(t["np"][:, 0], [e[0] for e in t["exact"]]).max() < 4 * dc.EPS * np.abs(t["np"]).max()
    d = dc.density_cases()
    assert (dc.frac_err(d["np"], d["exact"]) / d["np"]).max() < 4 * dc.EPS
    p = dc.pair_term_reference()
    for name, ref in p.items():
        assert ref["np_err"].max() < 6.0, name  # eps of the term's scale


# ---- census ----
@pytest.mark.parametrize("dp", dc.DP_BASELINE)
def test_spline_inputs_sit_on_the_edges_and_in_every_piece(dp):
    c = dc.spline_inputs(dp)
    q = c["r"] * c["kc"][1]  # as the device rounds it
    # q = 1 exactly and its neighbours: r moves in steps of ulp(h), which is up to two steps of q below 1 -- not every double next
    # to 1 is the product of some r, the nearest one is there
    assert np.any(q == 1.0) and np.any((q < 1.0) & (1.0 - q <= 2.0 ** -52)) and np.any((q > 1.0) & (q - 1.0 <= 2.0 ** -51))
    assert np.sum((q > 1.0) & (q < 1.0 + 2e-6)) >= 32 and np.sum((q < 1.0) & (q > 1.0 - 2e-6)) >= 32
    assert np.sum((q > 2.0 - 2e-6) & (c["r"] < 2.0 * c["h"])) >= 32
    assert na(2.0 * c["h"], 0.0) in c["r"]
    assert np.sum(q <= 1e-6) >= 32 and 0.0 in c["r"]
    assert np.sum(q < 1.0) > 1000 and np.sum((q >= 1.0) & (q < 2.0)) > 1000
    assert np.sum(c["near1"]) >= 100
    # outside: the zero branch of the two-piece forms and the clamp of spline_dW_sel
    r_out = dc.outside_q(dp)
    qo = r_out * c["kc"][1]
    assert 2.0 <= qo[0] <= na(2.0, 3.0) and 2.0 < qo[1] <= 2.0 + 2.0 ** -50 and abs(qo[2] - 3.0) < 1e-15 and abs(qo[3] - 1e6) < 1e-9
    # ... by the exact product too, which is what the device's fused 2 - r * inv_h sees; and each is the first such r
    exact_q = lambda r: Fraction(float(r)) * Fraction(c["kc"][1])
    assert all(exact_q(r) >= t for r, t in zip(r_out, (2, 2, 3, 10 ** 6))) and exact_q(na(r_out[0], 0.0)) < 2
    rb = dc.beyond_support(dp)
    assert rb[0] == na(2.0 * c["h"], np.inf) and np.all(np.diff(rb) > 0) and rb[-1] < 2.0 * c["h"] * (1 + 1e-15)
    # the exact reference is zero there and only there
    W, dW = dc.spline_exact(c["kc"], np.concatenate([rb, c["r"][:50]]))
    assert all(w == 0 for w in W[:4]) and all(w > 0 for w in W[4:]) and all(d == 0 for d in dW[:4])


def test_reciprocal_inputs_cover_the_stated_domains():
    x = dc.rcp_inputs()
    assert x.min() < 1e-11 and x.max() > 1e11 and all(dc.h_of(dp) in x for dp in dc.DP_ALL)
    assert 2.0 ** -40 in x and 2.0 ** 40 in x
    x = dc.rsqrt_inputs()
    assert x.min() == na(1e-24, 1.0) and 1e300 in x and np.all(x > 1e-24)
    assert 2.0 ** -77 in x and 2.0 ** -76 in x and 2.0 ** 39 in x and 2.0 ** 40 in x  # odd and even powers
    assert all((2 * dc.h_of(dp)) ** 2 in x for dp in dc.DP_ALL)
    dx, dy = dc.pair_geom_inputs()
    r2 = dx * dx + dy * dy
    assert np.all(r2 > 1e-24) and r2.min() < 1.1e-24
    assert np.any((dy == 0) & (dx > 0)) and np.any((dy == 0) & (dx < 0)) and np.any((dx == 0) & (dy > 0)) and np.any((dx == 0) & (dy < 0))
    assert np.any(np.abs(dx) > 1e10 * np.abs(dy)) and np.any(np.abs(dy) > 1e10 * np.abs(dx))


def test_pair_term_inputs_hold_the_named_pairs():
    c = dc.pair_term_inputs()
    e_dot_dv = ((c["vxi"] - c["ujx"]) * c["dx"] + (c["vyi"] - c["ujy"]) * c["dy"])
    assert e_dot_dv[0] > 0 and e_dot_dv[1] < 0  # separating, approaching
    face = -(c["acx"] * c["dx"] + c["acy"] * c["dy"])
    assert face[2] < 0 and face[3] == 0 and face[4] > 0
    assert np.sum(face > 0) > 100 and np.sum(face < 0) > 100
    r = np.hypot(c["dx"], c["dy"])
    assert np.all(r < 2 * c["h"]) and np.sum(r < c["h"]) > 100 and np.sum(r > c["h"]) > 100


def test_kgc_cases_enter_every_reachable_branch():
    k = dc.kgc_cases()
    A = k["A"]
    det = np.array([Fraction(a) * Fraction(d) - Fraction(b) * Fraction(c) for a, b, c, d in A])
    named = dict(zip(k["names"], range(len(k["names"]))))
    assert k["exact"][named["zero"]] == [1, 0, 0, 1]
    assert 0 < 1 - k["exact"][named["identity"]][0] < 1.01e-8  # (the regularisation: 1 / (1 + 1e-8))
    assert 0 < 1 - det[named["det_just_below_1"]] < 1e-15 and 0 < det[named["det_just_above_1"]] - 1 < 1e-15
    assert det[named["det_negative"]] < 0 and det[named["det_negative_large"]] < 0 and det[named["det_above_1"]] > 1
    assert abs(A[named["wall_truncated"]][3] - 0.5) < 0.05
    rnd = det[len(named):len(named) + 1000]
    assert np.sum(rnd > 1) > 50 and np.sum(rnd < 1) > 500 and min(rnd) >= Fraction(1, 5) and max(rnd) <= Fraction(6, 5)
    assert np.all(det[k["group"] == 1] == 0)  # rank one: B = I
    assert all(row == [1, 0, 0, 1] for row, g in zip(k["exact"], k["group"]) if g == 1)
    # the guards no finite input reaches (module docstring)
    n11 = A[:, 0] ** 2 + A[:, 2] ** 2 + 1e-8
    n22 = A[:, 1] ** 2 + A[:, 3] ** 2 + 1e-8
    n12 = A[:, 0] * A[:, 1] + A[:, 2] * A[:, 3]
    assert np.all(n11 * n22 - n12 * n12 >= 0.99e-16)


def test_small_formula_inputs_sit_on_their_switches():
    ul, ur, cf = dc.riemann_inputs()
    d = ul - ur
    assert np.sum(d < 0) > 100 and np.sum((d > 0) & (3 * d < cf)) > 100 and np.sum(3 * d > cf) > 100
    assert np.any(3.0 * d == cf) and np.any((d == 0) & (ul != 0)) and np.any((d == 0) & np.signbit(d))
    assert np.any(np.signbit(dc.riemann_numpy(ul, ur, cf)) & (dc.riemann_numpy(ul, ur, cf) == 0))  # -0.0 comes out as -0.0
    t = dc.transport_cases()
    fade = np.array([float(f) for f in t["fade_exact"]])
    raw = [100 * (Fraction(x) ** 2 + Fraction(y) ** 2) / Fraction(h) ** 2 for x, y, h in zip(t["inc_x"], t["inc_y"], t["h"])]
    assert sum(1 for f in raw if f == 1) >= 3                       # fade exactly 1 before the clamp
    assert any(0 < 1 - f < 1e-14 for f in raw) and any(0 < f - 1 < 1e-14 for f in raw)
    assert np.sum(fade < 1) > 1000 and sum(1 for f in raw if f > 1) > 1000 and np.any((t["inc_x"] == 0) & (t["inc_y"] == 0))
    dn = dc.density_cases()
    raw = [Fraction(a) * Fraction(r) * Fraction(s) + Fraction(b) * Fraction(r) ** 2 * Fraction(s) / Fraction(m) for a, b, m, r, s in zip(*dn["cols"])]
    t12 = Fraction(1e-12)
    assert sum(1 for v in raw if v == t12) >= 2 and any(0 < v - t12 < 1e-26 for v in raw) and any(0 < t12 - v < 1e-26 for v in raw)
    assert any(v < 0 for v in raw) and np.any(dn["cols"][1] < 0) and dn["floored"].sum() >= 5 and (~dn["floored"]).sum() > dn["n_random"]
    hs = dc.half_state_cases()
    raw = [Fraction(r) + Fraction(1, 2) * Fraction(s) * Fraction(d) for r, d, s in zip(*hs["cols"][:3])]
    t10 = Fraction(1e-10)
    assert any(v == t10 for v in raw) and any(0 < v - t10 < 1e-24 for v in raw) and any(0 < t10 - v < 1e-24 for v in raw)
    assert any(v < 0 for v in raw) and hs["floored"].sum() >= 3
    e = dc.eos_cases()
    assert sum(1 for v in e["exact"] if v == 0) == 2 and np.all(e["np"][[i for i, v in enumerate(e["exact"]) if v == 0]] == 0.0)


@pytest.mark.parametrize("DL", dc.DL_CASES)
def test_wrap_and_min_image_inputs_hold_the_listed_points(DL):
    w = dc.wrap_cases(DL)
    x = w["x"]
    for v in (-DL, -1e-17, 0.0, na(DL, 0.0), DL, na(DL, 2 * DL), 2.5 * DL, -0.25 * DL):
        assert v in x
    assert np.any((x == 0) & np.signbit(x))
    assert all(0 <= e < Fraction(DL) for e in w["exact"])
    # numpy's own result is DL exactly for the tiny negative inputs and for nothing else
    assert set(x[w["returns_DL"]]) == {-1e-17, -1e-300, -dc.ulp(DL) / 4}
    dx = dc.min_image_inputs(DL)
    half = 0.5 * DL
    for v in (half, -half, na(half, DL), na(-half, -DL)):
        assert v in dx
    folded = dc.min_image_numpy(dx, DL, half) != dx
    assert not folded[dx == half].any() and not folded[dx == -half].any() and folded[dx == na(half, DL)].all() and folded[dx == na(-half, -DL)].all()


@pytest.mark.parametrize("which", range(len(dc.GRIDS)))
def test_cell_inputs_sit_on_every_cell_edge(which):
    c = dc.cell_cases(which)
    assert set(c["cx"]) == set(range(c["ncx"])) and set(c["cy"]) == set(range(c["ncy"]))
    # (an edge x0 + k / inv_cs is no double in general: the inputs are the doubles around it)
    assert np.sum(c["edge_dist_x"] <= 2 * dc.ulp(c["DL"])) >= 3 * c["ncx"] and np.sum(c["edge_dist_y"] <= 2 * dc.ulp(c["DH"])) >= 3 * c["ncy"]
    assert np.all(np.diff(c["x"]) >= 0) and np.all(np.diff(c["y"]) >= 0)
    assert c["x"].min() < c["dpar"][0] and c["x"].max() > c["dpar"][0] + c["DL"]  # clamped at both ends


def test_next_dt_cases_bind_the_limit_they_name():
    for name, (t, tt, te, vmax, h, cf, dv, db) in dc.NEXT_DT_CASES.items():
        limits = dict(acoustic=0.25 * h / max(cf + vmax, 1e-12), viscous=dv, body=db, remain=min(tt - t, te - t))
        binding = min(limits, key=limits.get)
        if name.startswith("floor"):
            assert limits["remain"] <= 0 and dc.next_dt_numpy(t, tt, te, vmax, h, cf, dv, db, np.array(1)) == 1e-12
        elif name.startswith("remain"):
            assert binding == "remain" and 0 < limits["remain"] < 1e-4
        elif name in limits:
            assert binding == name
        d1 = dc.next_dt_numpy(t, tt, te, vmax, h, cf, dv, db, np.array(1))
        d3 = dc.next_dt_numpy(t, tt, te, vmax, h, cf, dv, db, np.array(3))
        assert d1 >= 1e-12 and d3 >= 1e-12
        if name == "advective_n3":
            assert abs(3 * d3 - 0.25 * h / vmax) < 1e-15 and 3 * d3 < 3 * limits["acoustic"]
        if name == "acoustic":
            assert abs(d3 - d1) < 1e-18  # three acoustic steps bind the outer step


def test_codec_cases_reach_bit_15_and_both_limits():
    k, i, n, per, lim = dc.encode_cases().astype(np.int64)
    d = k - i
    half = n >> 1
    d = np.where(per == 1, np.where(d > half, d - n, np.where(d < -half, d + n, d)), d)
    for limit in (dc.K_DELTA_MAX, dc.K_CODED_DELTA_MAX):
        m = lim == limit
        for v in (limit, -limit, limit + 1, -limit - 1):
            assert np.any(d[m] == v), (limit, v)
    assert set(n) == {2, 3, 101, 65535, 65536, 70001} and set(per) == {0, 1}
    assert np.any((per == 1) & (np.abs(k - i) > half))  # the fold itself
    assert dc.K_SLOT_CODES <= dc.K_CODE_BIAS - dc.K_CODED_DELTA_MAX and dc.K_CODE_BIAS + dc.K_CODED_DELTA_MAX <= 65535
    for lpp, cap in dense_cases.LIST_CAPACITY.items():
        a, rows, fl = dc.row_count_cases(lpp, cap)
        assert a[0].max() == cap and rows.max() == -(-cap // lpp) and rows.max() < (1 << 14)


def test_tile_layouts_hold_the_named_shapes():
    L = dc.tile_layouts()
    tot = [m[3] + m[4] + m[5] for m in L]
    for t in (dc.K_SLOT_CODES, dc.K_SLOT_CODES + 1, dc.K_FORCE_SLOTS, dc.K_FORCE_SLOTS + 1, 0):
        assert t in tot
    assert any(m[3] == 0 and m[4] and m[5] for m in L) and any(m[4] == 0 and m[3] and m[5] for m in L) and any(m[5] == 0 and m[3] and m[4] for m in L)
    assert any(m[0] + m[3] == m[1] or m[1] + m[4] == m[0] for m in L if m[3] and m[4])  # adjacent
    assert max(tot) > dc.K_SLOT_CODES
    for m in L:  # disjoint: every index is named by one slot
        idx = [dc.tile_index(m, sl) for sl in range(m[3] + m[4] + m[5])]
        assert len(set(idx)) == len(idx)
    m = dc.TILE_OVERLAPS[0]
    assert m[3] == 0 and m[0] == m[1]
    for m in dc.TILE_OVERLAPS:
        idx = [dc.tile_index(m, sl) for sl in range(m[3] + m[4] + m[5])]
        assert len(set(idx)) < len(idx)
    cases = dc.tile_ranges_cases()
    assert {c[1] for c in cases} == {1, 2, 3, 5} and {c[3] for c in cases} == {0, 1}
    for name, ncx, ncy, per, cell, start in cases:
        assert start[-1] == cell.size and np.all(np.diff(cell) >= 0)
    assert any(np.any(np.diff(start.reshape(-1)[::ncy]) == 0) for _, ncx, ncy, _, _, start in cases)  # an empty column


def test_bin_and_scale_inputs_sit_on_the_edges():
    for n_bins in (1, 7, 20, 213, 640):
        for DH in (1.0, 0.7):
            bin_w, y = dc.stats_bin_inputs(n_bins, DH)
            e = np.arange(n_bins + 1) * bin_w
            assert np.all(np.isin(e[e <= DH], y)) and 0.0 in y and DH in y and y.min() >= 0 and y.max() <= DH
            assert set(dc.profile_bin(y, DH, n_bins)) == set(range(n_bins))
    for n_bins in (1, 64, 500):
        bin_w, e2, r2 = dc.pair_bin_inputs(n_bins, 0.26)
        assert np.all(np.isin(e2[:-1], r2)) and np.all(np.isin(na(e2[1:], -np.inf), r2)) and r2.max() < e2[-1]
    v = dc.scale_vmax(0.065)
    assert np.isnan(v[-1]) and np.isinf(v[-2]) and 0.0 in v and 5e-324 in v and 1e300 in v
    assert sum(1 for x in v[:-2] if x > 0 and np.frexp(16.0 * x / 0.065)[0] == 0.5) >= 5  # 16 vmax / h a power of two
    assert sum(1 for x in v[:-2] if x > 0 and np.frexp(2.0 * x)[0] == 0.5) >= 5
    assert dc.stats_scales(0.0, 1) == (62 + 59, 62 + 118, 2.0 ** -59) and dc.stats_scales(np.nan, 1) == dc.stats_scales(0.0, 1)
    assert 2 ** 31 - 1 in dc.SCALE_N and 3 in dc.SCALE_N


# ---- the harness library ----
def test_harness_library_is_built_and_exports_its_entries(capi):
    assert os.path.exists(devtest.LIB_PATH), "build() makes csrc/libsphx_devtest.so"
    L = devtest.lib()
    for name in devtest.ENTRIES:
        assert getattr(L, name) is not None
    # its table and the Python side's list of operations are the same list
    info, n_ops = devtest.op_info(0)
    assert n_ops == len(devtest.OPS) and info == (1, 0, 1, 0)
    assert devtest.op_info(devtest.OP["C_CODED_INDEX"])[0] == (0, 9, 0, 1)
    assert devtest.op_info(devtest.OP["F_WALL_PRESSURE_ADD"])[0] == (11, 0, 2, 0)
    assert devtest.op_info(devtest.OP["B_QUANTISE"])[0] == (1, 1, 0, 2)
    assert devtest.lib().sphx_devtest_op_info(len(devtest.OPS), (ctypes.c_int * 4)()) == -1
    # the product library knows nothing of it
    assert not any("devtest" in name for name in capi.EXPORTS)
    assert not hasattr(capi.lib(), "sphx_devtest_formulas")


def test_harness_entries_refuse_bad_arguments_before_any_launch():
    bad = 1  # hipErrorInvalidValue
    assert devtest.call("F_RCP_NR", [[1.0, 2.0]], i=[[1, 2]], check=False) == bad              # a column too many
    assert devtest.call("L_GROUP_SUM", [np.ones(100)], ipar=[4], check=False) == bad            # not whole blocks
    assert devtest.call("L_GROUP_SUM", [np.ones(256)], ipar=[3], check=False) == bad            # no such lane group
    assert devtest.call("B_STATS_BIN", [[0.5]], dpar=[0.1], ipar=[0], check=False) == bad
    assert devtest.put_delta(np.zeros(8), 4, 4, [4], [0], [1], check=False) == bad             # row beyond the buffer
    assert devtest.put_delta(np.zeros(8), 4, 4, [0], [4], [1], check=False) == bad             # column beyond the stride
    assert devtest.tile_ranges(3, 2, 2, 1, [0, 1], [0, 1, 2, 2, 2], 2, 480, 1, check=False) == bad
    assert devtest.tile_ranges(2, 2, 2, 1, [0, 4], [0, 1, 2, 2, 2], 2, 480, 1, check=False) == bad   # a cell beyond the grid
    # one family's entry does not run another's operation
    L = devtest.lib()
    z = np.zeros(4)
    assert L.sphx_devtest_bins(devtest.OP["F_RCP_NR"], z.ctypes.data_as(devtest._dp), 1, None, 0, z.ctypes.data_as(devtest._dp), 1, None, 0,
                               4, None, 0, None, 0) == bad
