"""Field maps (include/sphx.h section 2e) without a GPU: the C ABI declares and exports the five entry points, the config
struct has the header's layout, the Python binding checks its arguments before anything reaches the library,
profile.shepard_field (the numpy form of the definition, the oracle of tests/test_gpu_field_map.py) has the properties the
definition promises, driver.field_figures is checked on synthetic maps with known answers, and driver.run refuses the
engine that has no device to accumulate on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from field_map_cases import void_case
from helpers import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD_SYMBOLS = ("sphx_ctx_field_map_enable", "sphx_ctx_field_map_disable", "sphx_ctx_field_map_reset",
                 "sphx_ctx_field_map_sample", "sphx_ctx_field_map_read")


def test_field_symbols_declared_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "sphx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    assert "sphx_field_map_config" in hdr
    for name in FIELD_SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)


def test_config_struct_matches_the_header(capi):
    hdr = open(os.path.join(ROOT, "include", "sphx.h")).read()
    body = re.search(r"typedef struct sphx_field_map_config \{(.*?)\} sphx_field_map_config;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = []
    for t, names in re.findall(r"(int32_t|double)\s+([\w\s,]+);", body):
        members += [(t, n.strip()) for n in names.split(",")]
    assert members == [("int32_t", "nx"), ("int32_t", "ny"), ("int32_t", "every"), ("int32_t", "with_walls"), ("double", "t_from")]
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    assert [(n, ctype[t]) for t, n in members] == list(capi.SphxFieldMapConfig._fields_)
    assert C.sizeof(capi.SphxFieldMapConfig) == 24 and capi.SphxFieldMapConfig.t_from.offset == 16


@pytest.mark.parametrize("kw", [dict(nx=1), dict(ny=1), dict(nx=-3), dict(ny=-1), dict(nx=2.0), dict(nx=True),
                                dict(nx=1 << 13, ny=(1 << 12) + 1), dict(every=0), dict(every=-2), dict(every=1.5),
                                dict(t_from=float("nan")), dict(t_from="soon"), dict(with_walls=2), dict(with_walls=-1),
                                dict(with_walls="yes")])
def test_binding_checks_the_config_first(capi, kw):
    with pytest.raises(capi.SphxError) as e:
        capi.field_map_config(**kw)
    assert e.value.identifier == "SPHX:Field:config" and e.value.code == capi.SPHX_ERR_ARG


def test_binding_config_and_shape(capi, cfgmod):
    cfg = capi.field_map_config(nx=1 << 13, ny=1 << 12, every=3, t_from=0.25, with_walls=True)
    assert (cfg.nx, cfg.ny, cfg.every, cfg.with_walls, cfg.t_from) == (1 << 13, 1 << 12, 3, 1, 0.25)
    cfg = capi.field_map_config()
    assert (cfg.nx, cfg.ny, cfg.every, cfg.with_walls, cfg.t_from) == (0, 0, 1, 0, 0.0)
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    assert capi.field_map_shape(prm) == (120, 40)
    assert capi.field_map_shape(prm, nx=7) == (7, 40) and capi.field_map_shape(prm, ny=9) == (120, 9)


# ---- profile.shepard_field ----
def _fluid(cfgmod, geom, dp=0.05, DL=3.0, seed=3, **kw):
    prm, parts = make_case(cfgmod, geom, dp=dp, DL=DL, jitter=0.2, seed=seed, developed=True, **kw)
    nf = parts["n_fluid"]
    return prm, parts, parts["pos"][:nf].copy(), parts["vel"][:nf].copy()


def test_shepard_constant_field_is_reproduced(cfgmod, geom, profmod):
    prm, parts, pos, vel = _fluid(cfgmod, geom)
    vel[:, 0], vel[:, 1] = 0.7310585786300049, -0.25
    f = profmod.shepard_field(pos, vel, prm.DL, prm.DH, prm.h, 120, 40)
    assert f["S0"].shape == f["u_x"].shape == (40, 120) and f["x"].shape == (120,) and f["y"].shape == (40,)
    assert np.array_equal(f["x"], np.linspace(0.0, prm.DL, 120)) and np.array_equal(f["y"], np.linspace(0.0, prm.DH, 40))
    hit = f["S0"] > 0
    assert hit.all()
    assert np.max(np.abs(f["u_x"][hit] - vel[0, 0])) <= 1e-14 and np.max(np.abs(f["u_y"][hit] + 0.25)) <= 1e-14


@pytest.mark.parametrize("dp,DL", [(0.05, 3.0), (0.1, 0.7), (0.1, 0.4)])
def test_shepard_is_periodic(cfgmod, geom, profmod, dp, DL):
    prm, parts, pos, vel = _fluid(cfgmod, geom, dp=dp, DL=DL)
    nx, ny = 2 * int(np.floor(DL / dp + 0.5)), 2 * int(np.floor(prm.DH / dp + 0.5))
    f = profmod.shepard_field(pos, vel, prm.DL, prm.DH, prm.h, nx, ny)
    bound = 1e-13 * max(np.max(np.abs(vel)), 1e-300)
    for k in ("u_x", "u_y"):
        assert np.max(np.abs(f[k][:, 0] - f[k][:, -1])) <= bound, k      # column 0 and nx - 1: the same physical line
    shifted = pos.copy()
    shifted[:, 0] += prm.DL
    g = profmod.shepard_field(shifted, vel, prm.DL, prm.DH, prm.h, nx, ny)
    for k in ("u_x", "u_y"):
        assert np.max(np.abs(f[k] - g[k])) <= bound, k
    assert np.max(np.abs(f["S0"] - g["S0"])) <= 1e-13 * np.max(f["S0"])


def test_shepard_void_nodes_have_no_weight(cfgmod, geom, profmod):
    prm, parts = void_case(cfgmod, geom)
    nf = parts["n_fluid"]
    pos, vel = parts["pos"][:nf], parts["vel"][:nf]
    nx, ny = 120, 40
    f = profmod.shepard_field(pos, vel, prm.DL, prm.DH, prm.h, nx, ny)
    X, Y = np.meshgrid(f["x"], f["y"])                      # [ny, nx]
    d2 = np.full((ny, nx), np.inf)
    for a in range(0, nf, 256):
        dx = X[..., None] - pos[None, None, a:a + 256, 0]
        dx -= prm.DL * np.round(dx / prm.DL)
        dy = Y[..., None] - pos[None, None, a:a + 256, 1]
        d2 = np.minimum(d2, np.min(dx * dx + dy * dy, axis=2))
    far = d2 >= (2.0 * prm.h) ** 2
    assert far.sum() >= 5 and not far[:, :40].any()            # (a disc of radius ~h of nodes around the centre)
    assert np.array_equal(f["S0"] == 0.0, far)
    assert np.all(np.isnan(f["u_x"][far])) and np.all(np.isfinite(f["u_x"][~far]))
    # nodes picked one by one give the whole grid's numbers (summed in another order: numpy's matrix product)
    nodes = np.array([0, ny - 1, nx * ny - 1, (nx // 2) * ny + ny // 2, 1234])
    sub = profmod.shepard_field(pos, vel, prm.DL, prm.DH, prm.h, nx, ny, nodes=nodes)
    for k in ("S0", "S1", "S2"):
        assert np.max(np.abs(sub[k] - f[k].T.ravel()[nodes])) <= 1e-13 * np.max(np.abs(f[k])), k


def test_shepard_wall_rows_enter_the_sums(cfgmod, geom, profmod):
    prm, parts, pos, vel = _fluid(cfgmod, geom)
    nf = parts["n_fluid"]
    wpos = parts["pos"][nf:]
    wvel = np.column_stack([np.full(len(wpos), 2.0), np.zeros(len(wpos))])
    a = profmod.shepard_field(pos, vel, prm.DL, prm.DH, prm.h, 120, 40)
    b = profmod.shepard_field(pos, vel, prm.DL, prm.DH, prm.h, 120, 40, wall_pos=wpos, wall_vel=wvel)
    inner = (a["y"] > 2.0 * prm.h + 1e-9) & (a["y"] < prm.DH - 2.0 * prm.h - 1e-9)
    for k in ("S0", "S1"):   # more than 2h from both walls nothing changes (but the order numpy sums in)
        assert np.max(np.abs(a[k][inner] - b[k][inner])) <= 1e-13 * np.max(np.abs(a[k])), k
    assert np.all(b["S0"][0] > a["S0"][0]) and np.all(b["u_x"][0] > a["u_x"][0])   # wall nodes feel the moving wall
    dp2 = prm.dp ** 2
    assert 0.3 < np.min(a["S0"][0]) * dp2 < 0.6 and np.min(b["S0"][0]) * dp2 > 0.8   # half a support / a whole one


# ---- driver.field_figures on synthetic maps ----
def _map(prm, nx, ny, u):
    return dict(x=np.linspace(0.0, prm.DL, nx), y=np.linspace(0.0, prm.DH, ny), u_x=u, u_y=np.zeros_like(u),
                count=np.ones_like(u), n_samples=1)


def test_figures_exact_parabola(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    nx, ny = 120, 40
    y = np.linspace(0.0, prm.DH, ny)
    u = np.repeat((prm.gravity_g / (2.0 * prm.nu) * y * (prm.DH - y))[:, None], nx, axis=1)
    f = driver.field_figures(prm, _map(prm, nx, ny, u))
    assert f["L2"] <= 1e-12 and f["x_spread"] == 0.0 and f["uy_rms"] == 0.0
    assert f["u_row_mean"].shape == (ny,) and f["U_max"] == prm.gravity_g * prm.DH ** 2 / (8.0 * prm.nu)
    rows = f["rows"]
    assert np.array_equal(rows, (y >= 2.0 * prm.h) & (y <= prm.DH - 2.0 * prm.h)) and rows.sum() >= ny - 14


def test_figures_find_a_bump_at_the_seam(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    nx, ny = 120, 40
    y = np.linspace(0.0, prm.DH, ny)
    u = np.repeat((prm.gravity_g / (2.0 * prm.nu) * y * (prm.DH - y))[:, None], nx, axis=1)
    u_max = prm.gravity_g * prm.DH ** 2 / (8.0 * prm.nu)
    u[ny // 2, 0] += 0.05 * u_max
    u[3, 77] = np.nan                                        # a node never sampled is left out, not propagated
    m = _map(prm, nx, ny, u)
    m["u_y"] = np.full_like(u, 0.01)
    f = driver.field_figures(prm, m)
    assert f["ix"] == 0 and f["iy"] == ny // 2
    np.testing.assert_allclose(f["x_spread"], 5.0 * (nx - 1) / nx, rtol=1e-9)   # the bump lifts its own row mean by 1/nx of it
    assert 0.0 < f["L2"] < 1e-3
    np.testing.assert_allclose(f["uy_rms"], 0.01, rtol=1e-12)


def test_driver_refuses_the_mex_engine(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0, end_time=0.01, output_interval=0.01)
    with pytest.raises(ValueError, match="resident"):
        driver.run(prm, engine="mex", field_from=0.0)


def test_figures_of_a_mirrored_flow(cfgmod, driver):
    """x -> DL - x, u_x -> -u_x, g -> -g: the same flow seen from behind.  L2, x_spread (in % of |U_max|) and uy_rms are equal
    and not negative, the bump is found at the mirrored node, U_max and the row means flip their sign.  (A spread divided
    by a signed U_max came out negative for every leftward flow and passed any `x_spread < tol`.)"""
    nx, ny = 120, 40
    rng = np.random.default_rng(5)
    noise = 0.01 * rng.standard_normal((ny, nx))
    uy = 0.02 * rng.standard_normal((ny, nx))
    out = {}
    for sign in (1, -1):
        prm = cfgmod.params_from_values(dp=0.05, DL=3.0, U_bulk=sign * 0.666667)
        y = np.linspace(0.0, prm.DH, ny)
        u = np.repeat((prm.gravity_g / (2.0 * prm.nu) * y * (prm.DH - y))[:, None], nx, axis=1) + sign * noise
        u[ny // 2, 2] += sign * 0.05
        u[3, 77] = np.nan
        m = _map(prm, nx, ny, u if sign > 0 else u[:, ::-1].copy())
        m["u_y"] = uy if sign > 0 else uy[:, ::-1].copy()
        out[sign] = driver.field_figures(prm, m)
    a, b = out[1], out[-1]
    assert a["U_max"] > 0 and b["U_max"] == -a["U_max"]
    assert (a["ix"], a["iy"]) == (2, ny // 2) and (b["ix"], b["iy"]) == (nx - 3, ny // 2)
    assert a["x_spread"] > 4.0                        # 5 % of U_max = 1 on top of the noise
    for k in ("L2", "x_spread", "uy_rms"):
        assert a[k] > 0 and b[k] >= 0, (k, a[k], b[k])
        assert abs(a[k] - b[k]) <= 1e-12 * a[k], (k, a[k], b[k])
    ok = ~np.isnan(a["u_row_mean"])
    np.testing.assert_allclose(b["u_row_mean"][ok], -a["u_row_mean"][ok], rtol=1e-12)
    assert np.array_equal(b["u_exact"], -a["u_exact"])
