"""Cases, point sets and comparisons shared by tests/test_probes_host.py, tests/test_gpu_probes.py and
tests/test_gpu_batch_probes.py (point probes, include/sphx.h sections 2h / 2i)."""
import numpy as np

FIELDS = ("weight", "u_x", "u_y", "rho")
SERIES = ("step", "t") + FIELDS
WAVES = 16        # probes of a workgroup of k_point_probes (csrc/sphx_probes.hpp, kProbeBlock / 64): up to here no ticket
BOUND = 1e-12     # a probe sums up to about 150 non-negative weights, each product rounded to 1.1e-16, then divides once:
                  # about 1e-13 of the largest |value| of a column (tests/test_gpu_field_map.py's bound and argument)

# name: (dp, DL, context options, make_case options) -- the field map's small cases
CASES = {
    "dp05_auto": (0.05, 3.0, dict(), dict()),                          # 1 200 particles, compact kernels
    "dp025_walk": (0.025, 1.5, dict(lanes_per_particle=4), dict()),
    "dp05_dynamic": (0.05, 3.0, dict(dynamic_rebin=1), dict()),
    "dp025_dual": (0.025, 1.5, dict(lanes_per_particle=16, dual_rate=2), dict()),
    "two_cols": (0.1, 0.6, dict(), dict()),                            # two cell columns
    "one_col": (0.1, 0.4, dict(), dict(developed=False)),              # one column, two images within 2h
    "dp01_multi": (0.01, 3.0, dict(), dict()),                         # 30 k particles
    # a skin of 2 h: cells 5.2 dp wide hold ~27 particles, a column run of three ~80 -- more than a wave, a lane takes two
    "dp05_wide_skin": (0.05, 3.0, dict(rebuild_every=16, skin_h=2.0), dict()),
}


def case(maker, cfgmod, geom, name, seed=11):
    """(prm, parts, context options) of CASES[name] from helpers.make_case or helpers.make_variant"""
    dp, DL, kw, mk = CASES[name]
    prm, parts = maker(cfgmod, geom, **dict(dict(dp=dp, DL=DL, jitter=0.2, seed=seed, developed=True), **mk))
    return prm, parts, kw


def cell_geometry(prm, parts, ctx):
    """(ncx, ncy, column width, row height, y of row 0) of the context's cell grid"""
    info = ctx.info()
    cs = 2.0 * prm.h + ctx.grid_policy()["skin"]
    return info["n_cell_x"], info["n_cell_y"], prm.DL / info["n_cell_x"], cs, float(np.min(parts["pos"][:, 1]))


def random_points(prm, n, seed):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.random(n) * prm.DL, rng.random(n) * prm.DH])


def special_points(prm, grid, pos_fluid):
    """The places a probe can go wrong: the seam (x = 0, DL, within 1e-12 of DL, -DL, beyond DL), both wall lines, the channel's
    corners, cell corners (both coordinates multiples of the cell size), a particle's own position."""
    ncx, ncy, csx, csy, y_min = grid
    DL, DH = prm.DL, prm.DH
    rows = [j for j in range(ncy + 1) if 0.0 <= y_min + j * csy <= DH]
    pts = [(0.0, 0.5 * DH), (DL, 0.5 * DH), (DL - 5e-13, 0.31 * DH), (-DL, 0.5 * DH), (2.5 * DL, 0.4 * DH), (-0.25 * DL, 0.6 * DH),
           (0.3 * DL, 0.0), (0.3 * DL, DH), (0.0, 0.0), (DL, DH), (0.0, DH)]
    pts += [(csx * (k % ncx), y_min + csy * j) for k, j in zip((0, 1, ncx - 1), (rows[0], rows[len(rows) // 2], rows[-1]))]
    inside = np.flatnonzero((pos_fluid[:, 1] > 0.1 * DH) & (pos_fluid[:, 1] < 0.9 * DH))
    pts += [tuple(pos_fluid[inside[17]]), tuple(pos_fluid[inside[len(inside) // 2]])]
    return np.array(pts, dtype=np.float64)


def point_sets(prm, grid, pos_fluid):
    """name -> points [P, 2]: P = 1, one below / at / one above a workgroup's waves, and 300 (19 workgroups draw the ticket)
    with the special points among them."""
    sp = special_points(prm, grid, pos_fluid)
    many = np.concatenate([sp, random_points(prm, 300 - len(sp), 5)])
    return {"one": random_points(prm, 1, 1), f"{WAVES - 1}": random_points(prm, WAVES - 1, 2), f"{WAVES}": random_points(prm, WAVES, 3),
            f"{WAVES + 1}": np.concatenate([sp[:4], random_points(prm, WAVES + 1 - 4, 4)]), "300": many}


def numpy_probes(profmod, prm, parts, state, points, with_walls=False):
    """profile.shepard_points of a downloaded state (pos, vel) with the masses of parts"""
    nf = parts["n_fluid"]
    walls = dict(wall_pos=parts["pos"][nf:], wall_vel=parts["wall_vel"][nf:]) if with_walls else {}
    return profmod.shepard_points(state["pos"][:nf], state["vel"][:nf], parts["mass"][:nf], prm.DL, prm.h, prm.dp, points, **walls)


def assert_values_match(got, want, what, row=None, bound=BOUND):
    """the four fields of record `row` of a probes dict (None: [P] arrays) against [P] arrays: NaN exactly where `want` has NaN,
    otherwise within bound of the column's largest |value|"""
    for k in FIELDS:
        g = np.asarray(got[k] if row is None else got[k][row], dtype=np.float64)
        w = np.asarray(want[k], dtype=np.float64)
        assert g.shape == w.shape, f"{what}: {k} {g.shape} {w.shape}"
        assert np.array_equal(np.isnan(g), np.isnan(w)), f"{what}: {k} NaN pattern"
        ok = ~np.isnan(w)
        if not ok.any():
            continue
        scale = max(float(np.max(np.abs(w[ok]))), 1e-300)
        err = float(np.max(np.abs(g[ok] - w[ok])))
        print(f"{what}: {k} off by {err / scale:.3e} of the largest |value|")
        assert err <= bound * scale, f"{what}: {k} off by {err / scale:.3e} of the largest |value|"


def assert_series_identical(a, b, what):
    """two probes dicts bit for bit (NaN equal to NaN), counters included"""
    assert np.array_equal(a["points"], b["points"]), what + ": points"
    for k in SERIES:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k}"
    assert a["n_dropped"] == b["n_dropped"], what


def assert_series_close(a, b, what, bound=BOUND):
    """the same records up to summation order: step and t exact, the fields within bound of a record's largest |value|"""
    assert np.array_equal(a["step"], b["step"]) and np.array_equal(a["t"], b["t"]) and a["n_dropped"] == b["n_dropped"], what
    for r in range(len(a["step"])):
        assert_values_match(a, {k: b[k][r] for k in FIELDS}, f"{what}: record {r}", row=r, bound=bound)
