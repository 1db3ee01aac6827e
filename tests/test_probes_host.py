"""Point probes (include/sphx.h sections 2h / 2i) without a GPU: the C ABI declares and exports the eight entry points, the
two macros and the config struct, the ctypes struct has the header's layout, the Python binding checks its arguments before
anything reaches the library, profile.shepard_points (the numpy form of the definition, the oracle of
tests/test_gpu_probes.py) agrees with profile.shepard_field on map nodes and with a brute-force double loop, folds x as the
definition says and reports a void as "no value", and driver.probe_figures is checked on a synthetic series with known
answers."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from field_map_cases import void_case
from helpers import make_case, make_variant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SYMBOLS = tuple(f"sphx_{who}_probes_{what}" for who in ("ctx", "batch") for what in ("enable", "disable", "sample", "read"))


def test_probe_symbols_declared_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "sphx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    assert len(PROBE_SYMBOLS) == 8
    for name in PROBE_SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)
    assert "sphx_probes_config" in hdr
    assert re.search(r"^#define SPHX_PROBE_FIELDS 4\s*$", hdr, re.M) and re.search(r"^#define SPHX_PROBE_MAX_POINTS 4096\s*$", hdr, re.M)
    assert capi.PROBE_FIELDS == ("weight", "u_x", "u_y", "rho") and capi.PROBE_MAX_POINTS == 4096


def test_config_struct_matches_the_header(capi):
    hdr = open(os.path.join(ROOT, "include", "sphx.h")).read()
    body = re.search(r"typedef struct sphx_probes_config \{(.*?)\} sphx_probes_config;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = []
    for t, names in re.findall(r"(int32_t|const double \*|double)\s*([\w\s,]+);", body):
        members += [(t, n.strip()) for n in names.split(",")]
    assert members == [("int32_t", "n_points"), ("int32_t", "every"), ("int32_t", "capacity"), ("int32_t", "with_walls"),
                       ("double", "t_from"), ("const double *", "points")]
    ctype = {"int32_t": C.c_int32, "double": C.c_double, "const double *": C.POINTER(C.c_double)}
    assert [(n, ctype[t]) for t, n in members] == list(capi.SphxProbesConfig._fields_)
    assert C.sizeof(capi.SphxProbesConfig) == 32 and capi.SphxProbesConfig.t_from.offset == 16 and capi.SphxProbesConfig.points.offset == 24


@pytest.mark.parametrize("kw", [dict(points=None), dict(points=[]), dict(points=[1.0, 2.0]), dict(points=[[0.1, 0.2, 0.3]]),
                                dict(points=np.zeros((4097, 2))), dict(points=[[float("nan"), 0.5]]), dict(points=[[0.5, float("inf")]]),
                                dict(points=[[0.5, -1e-9]]), dict(points=[[0.5, 1.0 + 1e-9]]), dict(points="here"), dict(every=0),
                                dict(every=-2), dict(every=1.5), dict(capacity=0), dict(capacity=2.0), dict(capacity=(1 << 25) + 1),
                                dict(capacity=1 << 24, n_members=3), dict(t_from=float("nan")), dict(t_from=float("inf")),
                                dict(t_from="soon"), dict(with_walls=2), dict(with_walls=-1), dict(with_walls="yes")])
def test_binding_checks_the_config_first(capi, cfgmod, kw):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    assert prm.DH == 1.0
    args = dict(dict(points=[[0.5, 0.5]]), **kw)
    with pytest.raises(capi.SphxError) as e:
        capi.probes_config(prm, **args)
    assert e.value.identifier == "SPHX:Probe:config" and e.value.code == capi.SPHX_ERR_ARG


def test_binding_config_folds_and_copies(capi, cfgmod):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    given = np.array([[0.0, 0.0], [3.0, 1.0], [-3.0, 0.5], [7.5, 0.25], [-0.75, 0.75], [3.0 - 5e-13, 0.5], [-1e-20, 0.5]])
    cfg, pts = capi.probes_config(prm, given, every=3, capacity=(1 << 27) // 28, t_from=0.25, with_walls=True)
    assert (cfg.n_points, cfg.every, cfg.capacity, cfg.with_walls, cfg.t_from) == (7, 3, (1 << 27) // 28, 1, 0.25)   # the largest capacity 7 points allow
    assert np.array_equal(pts[:, 0], [0.0, 0.0, 0.0, 1.5, 2.25, 3.0 - 5e-13, 0.0]) and np.array_equal(pts[:, 1], given[:, 1])
    assert np.all((pts[:, 0] >= 0.0) & (pts[:, 0] < prm.DL)) and given[1, 0] == 3.0      # folded into [0, DL); the input is left alone
    assert [cfg.points[k] for k in range(4)] == [0.0, 0.0, 0.0, 1.0]                      # (x, y) rows
    cfg, pts = capi.probes_config(prm, [(0.5, 0.5)])
    assert (cfg.n_points, cfg.every, cfg.capacity, cfg.with_walls, cfg.t_from) == (1, 1, 65536, 0, 0.0)
    d = capi.probes_dict(pts, np.array([[3.0, 0.1], [6.0, 0.2]]), np.arange(8.0).reshape(2, 1, 4), 5)
    assert d["step"].dtype == np.int64 and list(d["step"]) == [3, 6] and list(d["t"]) == [0.1, 0.2] and d["n_dropped"] == 5
    assert [d[k].tolist() for k in capi.PROBE_FIELDS] == [[[0.0], [4.0]], [[1.0], [5.0]], [[2.0], [6.0]], [[3.0], [7.0]]]


# ---- profile.shepard_points ----
def test_shepard_points_on_map_nodes_is_shepard_field(cfgmod, geom, profmod):
    prm, parts = make_variant(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.2, seed=3, developed=True)
    nf = parts["n_fluid"]
    pos, vel, mass = parts["pos"][:nf], parts["vel"][:nf], parts["mass"][:nf]
    nx, ny = 61, 21
    rng = np.random.default_rng(2)
    nodes = np.unique(np.concatenate([np.arange(ny), rng.choice((nx - 1) * ny, size=400, replace=False)]))  # column 0 and inner nodes
    xs, ys = profmod.field_map_nodes(prm.DL, prm.DH, nx, ny)
    pts = np.column_stack([xs[nodes // ny], ys[nodes % ny]])
    for walls in (dict(), dict(wall_pos=parts["pos"][nf:], wall_vel=parts["wall_vel"][nf:])):
        f = profmod.shepard_field(pos, vel, prm.DL, prm.DH, prm.h, nx, ny, nodes=nodes, **walls)
        p = profmod.shepard_points(pos, vel, mass, prm.DL, prm.h, prm.dp, pts, **walls)
        assert np.array_equal(p["points"], pts)
        for a, b in ((p["u_x"], f["u_x"]), (p["u_y"], f["u_y"]), (p["S0"], f["S0"]), (p["weight"], f["S0"] * prm.dp ** 2)):
            assert not np.any(np.isnan(b)) and np.max(np.abs(a - b)) <= 1e-15 * np.max(np.abs(b))
    assert np.all(p["weight"][:ny][[0, -1]] > 0.8)   # with walls a wall node has a full neighbourhood


def test_shepard_points_rho_is_the_brute_force_sum(cfgmod, geom, profmod):
    prm, parts = make_variant(cfgmod, geom, dp=0.1, DL=1.0, jitter=0.2, seed=5, developed=True)
    nf = parts["n_fluid"]
    pick = np.random.default_rng(4).choice(nf, size=min(nf, 200), replace=False)
    pos, vel, mass = parts["pos"][:nf][pick], parts["vel"][:nf][pick], parts["mass"][:nf][pick]
    assert len(pos) in (100, 200) and np.ptp(mass) > 0.1 * np.mean(mass)
    pts = np.column_stack([np.random.default_rng(6).random(40) * prm.DL, np.random.default_rng(7).random(40) * prm.DH])
    got = profmod.shepard_points(pos, vel, mass, prm.DL, prm.h, prm.dp, pts, wall_pos=parts["pos"][nf:], wall_vel=parts["wall_vel"][nf:])
    h, sigma = prm.h, 10.0 / (7.0 * math.pi * prm.h ** 2)
    want = np.zeros(len(pts))
    for k, (x, y) in enumerate(pts):
        for (px, py), m in zip(pos, mass):        # fluid only: the walls never enter rho
            dx = x - px
            dx = dx - prm.DL if dx > 0.5 * prm.DL else (dx + prm.DL if dx < -0.5 * prm.DL else dx)
            r = math.sqrt(dx * dx + (y - py) ** 2)
            q = r / h
            if r * r < (2.0 * h) ** 2:
                want[k] += m * sigma * ((1.0 - 1.5 * q * q + 0.75 * q ** 3) if q < 1.0 else 0.25 * (2.0 - q) ** 3)
    assert np.max(want) > 0 and np.max(np.abs(got["rho"] - want)) <= 1e-13 * np.max(want)


def test_shepard_points_folds_x(cfgmod, geom, profmod):
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.2, seed=3, developed=True)
    nf = parts["n_fluid"]
    pos, vel, mass = parts["pos"][:nf], parts["vel"][:nf], parts["mass"][:nf]
    ys = (0.0, 0.37, 1.0)
    out = [profmod.shepard_points(pos, vel, mass, prm.DL, prm.h, prm.dp, [(x, y) for y in ys]) for x in (0.0, prm.DL, -prm.DL)]
    for o in out:
        assert np.all(o["points"][:, 0] == 0.0) and not np.any(np.signbit(o["points"][:, 0]))
    for k in ("S0", "weight", "u_x", "u_y", "rho"):
        assert out[0][k].tobytes() == out[1][k].tobytes() == out[2][k].tobytes(), k


def test_shepard_points_void_is_no_value(cfgmod, geom, profmod):
    prm, parts = void_case(cfgmod, geom)
    nf = parts["n_fluid"]
    pts = [(0.5 * prm.DL, 0.5 * prm.DH), (0.5 * prm.DL + 0.5 * prm.h, 0.5 * prm.DH), (0.25 * prm.DL, 0.5 * prm.DH)]
    got = profmod.shepard_points(parts["pos"][:nf], parts["vel"][:nf], parts["mass"][:nf], prm.DL, prm.h, prm.dp, pts)
    for k in (0, 1):
        assert np.isnan(got["u_x"][k]) and np.isnan(got["u_y"][k]) and got["weight"][k] == 0.0 and got["rho"][k] == 0.0
    assert np.isfinite(got["u_x"][2]) and got["weight"][2] > 0.8 and got["rho"][2] > 0.8 * prm.rho0


# ---- driver.probe_figures ----
def test_probe_figures_on_a_synthetic_series(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    rng = np.random.default_rng(8)
    n, dt0, f0, amp, ux0 = 2000, 1e-3, 37.0, 0.04, 0.731
    t = np.cumsum(dt0 * (1.0 + 0.3 * (rng.random(n) * 2 - 1)))      # non-uniform steps
    pts = np.array([[0.5, 0.25], [1.0, 0.5]])
    u_y = np.column_stack([amp * np.sin(2 * np.pi * f0 * t), 0.5 * amp * np.sin(2 * np.pi * 2 * f0 * t + 0.3)])
    rho = prm.rho0 * (1.0 + 0.01 * np.column_stack([np.sin(2 * np.pi * 3 * f0 * t), np.sin(2 * np.pi * f0 * t)]))
    probes = dict(points=pts, step=np.arange(1, n + 1), t=t, weight=np.ones((n, 2)), u_x=np.full((n, 2), ux0), u_y=u_y, rho=rho,
                  n_dropped=0)
    fig = driver.probe_figures(prm, probes)
    f_bin = fig["f_bin"]
    assert fig["n_records"] == n and abs(f_bin - 1.0 / (t[-1] - t[0])) < 0.01 * f_bin
    assert abs(fig["f_peak_uy"][0] - f0) <= f_bin and abs(fig["f_peak_uy"][1] - 2 * f0) <= f_bin
    assert abs(fig["f_peak_p"][0] - 3 * f0) <= f_bin and abs(fig["f_peak_p"][1] - f0) <= f_bin
    assert abs(fig["u_y_rms"][0] - amp / np.sqrt(2)) <= 0.01 * amp / np.sqrt(2)
    assert abs(fig["u_y_rms"][1] - 0.5 * amp / np.sqrt(2)) <= 0.01 * 0.5 * amp / np.sqrt(2)
    assert np.all(fig["u_x_mean"] == ux0) and np.all(fig["u_x_rms"] == 0.0)              # exact
    assert abs(fig["p_rms"][0] - 0.01 * prm.p0 / np.sqrt(2)) <= 0.01 * 0.01 * prm.p0 / np.sqrt(2)
    y = pts[:, 1]
    assert np.allclose(fig["u_exact"], prm.gravity_g / (2 * prm.nu) * y * (prm.DH - y), rtol=1e-15)
    assert fig["f_acoustic"] == prm.c_f * abs(prm.gravity_g * prm.DH ** 2 / (12 * prm.nu)) / (2 * prm.DH)
    late = driver.probe_figures(prm, probes, t_from=t[n // 2])
    assert late["n_records"] == n - n // 2 and abs(late["f_peak_uy"][0] - f0) <= late["f_bin"]
    void = dict(probes, u_y=np.where(np.arange(n)[:, None] == 5, np.nan, u_y))
    assert np.all(np.isnan(driver.probe_figures(prm, void)["f_peak_uy"]))
    empty = driver.probe_figures(prm, probes, t_from=1e9)
    assert empty["n_records"] == 0 and np.all(np.isnan(empty["u_x_mean"])) and np.all(np.isnan(empty["f_peak_p"]))


def test_driver_refuses_probes_without_a_device_engine(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.1, DL=1.0, end_time=0.001, output_interval=0.001)
    with pytest.raises(ValueError, match="probe_points"):
        driver.run(prm, engine="mex", probe_points=[(0.5, 0.5)])
