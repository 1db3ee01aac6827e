"""Mode amplitudes (include/sphx.h sections 2t / 2u) without a GPU: the library exports the eight entry points and the ctypes
struct has the header's layout, the binding checks its arguments first, profile.mode_sums is the definition (its exact
identities on the lattice at rest, the sine coefficients of the analytic parabola, its own rounding error against
np.longdouble), driver.mode_figures gives the known answers on a series built from the start-up solution, and the oracle's own
trajectory gives the distance from the closed form that tests/test_gpu_modes.py holds the device to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mode_cases as mc
from helpers import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = tuple(f"sphx_{who}_modes_{what}" for who in ("ctx", "batch") for what in ("enable", "disable", "sample", "read"))


# 1 ---------------------------------------------------------------------------------------------------------------
def test_symbols_declared_and_exported(capi, profmod):
    raw = open(os.path.join(ROOT, "include", "sphx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    assert len(SYMBOLS) == 8
    for name in SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)
    assert not any("slab" in n and "modes" in n for n in declared)  # slab rings are the next step
    assert re.search(r"^#define SPHX_MODE_FIELDS 3\b", hdr, re.M) and re.search(r"^#define SPHX_MODE_BASES 4\b", hdr, re.M)
    assert re.search(r"^#define SPHX_MODES_MAX 16\s*$", hdr, re.M) and capi.MODES_MAX == 16
    assert capi.MODE_FIELDS == profmod.MODE_FIELDS == mc.FIELDS and capi.MODE_BASES == profmod.MODE_BASES == mc.BASES


def test_config_struct_matches_the_header(capi):
    hdr = open(os.path.join(ROOT, "include", "sphx.h")).read()
    body = re.search(r"typedef struct sphx_modes_config \{(.*?)\} sphx_modes_config;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = []
    for t, names in re.findall(r"(int32_t|double)\s*([\w\s,\[\]]+);", body):
        members += [(t, n.strip()) for n in names.split(",")]
    assert members == [("int32_t", "mx"), ("int32_t", "ny"), ("int32_t", "every"), ("int32_t", "capacity"), ("double", "t_from")]
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    assert [(n, ctype[t]) for t, n in members] == list(capi.SphxModesConfig._fields_)
    S = capi.SphxModesConfig
    assert (C.sizeof(S), S.ny.offset, S.every.offset, S.capacity.offset, S.t_from.offset) == (24, 4, 8, 12, 16)


@pytest.mark.parametrize("kw", [dict(mx=-1), dict(mx=17), dict(mx=2.5), dict(ny=-1), dict(ny=17), dict(ny="8"), dict(every=0), dict(every=-2),
                                dict(every=1.5), dict(capacity=0), dict(capacity=-3), dict(capacity=2.0), dict(t_from=float("nan")),
                                dict(t_from="soon"),
                                dict(capacity=(1 << 27) // 540 + 1),                       # (4, 8): 45 modes x 12 = 540 doubles a record
                                dict(mx=16, ny=16, capacity=(1 << 27) // 3468 + 1),        # 289 modes x 12 = 3 468
                                dict(capacity=(1 << 27) // (4 * 540) + 1, n_members=4)])
def test_binding_checks_the_config_first(capi, kw):
    with pytest.raises(capi.SphxError) as e:
        capi.modes_config(**kw)
    assert e.value.identifier == "SPHX:Modes:config" and e.value.code == capi.SPHX_ERR_ARG


def test_binding_accepts_the_limits(capi):
    cfg = capi.modes_config()
    assert (cfg.mx, cfg.ny, cfg.every, cfg.capacity, cfg.t_from) == (4, 8, 1, 4096, 0.0)
    cfg = capi.modes_config(mx=16, ny=16, every=7, capacity=(1 << 27) // 3468, t_from=-1.0)
    assert (cfg.mx, cfg.ny, cfg.every, cfg.capacity, cfg.t_from) == (16, 16, 7, (1 << 27) // 3468, -1.0)
    cfg = capi.modes_config(mx=0, ny=0, capacity=(1 << 27) // (4 * 12), n_members=4)
    assert (cfg.mx, cfg.ny) == (0, 0)


# 2 ---------------------------------------------------------------------------------------------------------------
def test_definition_on_the_lattice_at_rest(cfgmod, geom, profmod):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    parts = geom.init_particles(prm)
    nf = parts["n_fluid"]
    S = profmod.mode_sums(parts["pos"][:nf], parts["vel"][:nf], prm.DL, prm.DH, 16, 16)
    assert S["n"].shape == S["ux"].shape == S["uy"].shape == (17, 17, 4)
    mc.assert_exact_identities(S, nf, "lattice at rest")
    assert np.all(S["ux"] == 0.0) and np.all(S["uy"] == 0.0) and S["abs_n"] == float(nf) and S["abs_ux"] == 0.0
    # the lattice has 60 columns in x: no mode m <= 16 of it survives the sum over a row.  Measured 8.1e-13.
    worst = float(np.max(np.abs(S["n"][1:, 0, :])))
    print(f"lattice at rest: largest |n[m > 0, 0, :]| = {worst:.3e}")
    assert worst <= 1e-9


# measured by the test below, in U_max: the midpoint rule's error, which grows with n and falls 16-fold with half the spacing
PARABOLA_MEASURED = {0.05: {1: 2.296e-6, 3: 7.008e-6, 5: 1.210e-5, 7: 1.786e-5},
                     0.025: {1: 1.432e-7, 3: 4.316e-7, 5: 7.256e-7, 7: 1.029e-6}}
# even n: zero by symmetry up to the rounding of the sum -- N terms of at most U_max, each rounded to 1.1e-16 of itself, times
# 2 / N: a few 1e-16 U_max (measured: at most 5.4e-16).  Derived, not measured: 64 roundings of 1.1e-16.
PARABOLA_EVEN = 64 * 1.1e-16


@pytest.mark.parametrize("dp", [0.05, 0.025])
def test_sine_coefficients_of_the_parabola(cfgmod, geom, profmod, dp):
    """The lattice with u_x = g / (2 nu) y (DH - y) at every particle: (2 / N) ux[0, n, cs] is the midpoint rule for b_n =
    32 U_max / (n pi)^3 (odd n) and 0 (even n, by the lattice's symmetry about DH / 2).  The bound is twice the deviation this
    test itself measured, in U_max, written beside it: PARABOLA_MEASURED."""
    prm = cfgmod.params_from_values(dp=dp, DL=3.0)
    parts = geom.init_particles(prm)
    nf = parts["n_fluid"]
    pos = parts["pos"][:nf]
    vel = np.zeros((nf, 2))
    vel[:, 0] = prm.gravity_g / (2.0 * prm.nu) * pos[:, 1] * (prm.DH - pos[:, 1])
    u_max = prm.gravity_g * prm.DH ** 2 / (8.0 * prm.nu)
    S = profmod.mode_sums(pos, vel, prm.DL, prm.DH, 0, 8)
    b = 2.0 / nf * S["ux"][0, :, 2]
    for n in range(1, 9):
        exact = 32.0 * u_max / (n * np.pi) ** 3 if n % 2 else 0.0
        dev = abs(b[n] - exact) / u_max
        print(f"dp {dp}: b_{n} = {b[n]!r}, exact {exact!r}, deviation {dev:.3e} U_max")
        if n % 2:
            assert dev <= 2.0 * PARABOLA_MEASURED[dp][n], (n, dev)
        else:
            assert dev <= PARABOLA_EVEN, (n, dev)
    assert np.allclose(profmod.mode_b_exact(np.arange(9), 1e9, prm.gravity_g, prm.nu, prm.DH)[1::2],
                       [32.0 * u_max / (n * np.pi) ** 3 for n in (1, 3, 5, 7)], rtol=1e-14)


def test_floating_point_bound(cfgmod, geom, profmod):
    """FP_DEVIATION: the float64 definition against the same in np.longdouble, in units of sum |q_i|."""
    worst = 0.0
    for dp in (0.05, 0.025):
        prm, parts = make_case(cfgmod, geom, dp=dp, DL=3.0, jitter=0.2, seed=11, developed=True)
        nf = parts["n_fluid"]
        a = mc.numpy_modes(profmod, prm, parts["pos"][:nf], parts["vel"][:nf], 16, 16)
        b = mc.numpy_modes(profmod, prm, parts["pos"][:nf], parts["vel"][:nf], 16, 16, acc=np.longdouble)
        dev, f = mc.deviation(a, b)
        print(f"dp {dp}: float64 against longdouble: {dev:.3e} of sum |q| ({f})")
        worst = max(worst, dev)
    assert np.finfo(np.longdouble).eps < 1e-18  # (an extended type: the comparison says something)
    assert worst <= mc.FP_DEVIATION
    assert mc.BOUND == 1e-12


def test_scales(profmod):
    s = profmod.mode_scales(0.3, 1200)
    assert s == dict(s0=62 - 11, s1=62 - 11 - 0, bound=1.0)  # 2 * 0.3 = 0.6 < 2^0, 1200 <= 2^11
    s = profmod.mode_scales(0.5, 1 << 11)
    assert s == dict(s0=51, s1=50, bound=2.0)                # 2 * 0.5 = 1 = 2^0 is not < 2^0
    assert profmod.mode_scales(float("nan"), 1)["bound"] == 2.0 ** -59 and profmod.mode_scales(0.0, 1)["s0"] == 62


# 3 ---------------------------------------------------------------------------------------------------------------
def test_mode_figures_of_an_exact_series(cfgmod, driver, profmod):
    """A series built from the closed form: ux[:, 0, n, cs] = (N / 2) b_n(t) exactly, every other amplitude constant.  The fit
    is a least-squares line through log of one exponential: it returns tau_exact to the rounding of the logs, 1e-9 relative."""
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    N, mx, ny = 1200, 2, 8
    t = np.linspace(0.0, 2.0, 401)[1:]
    n = np.arange(ny + 1)
    ux = np.zeros((len(t), mx + 1, ny + 1, 4))
    ux[:, 0, :, 2] = 0.5 * N * profmod.mode_b_exact(n[None, :], t[:, None], prm.gravity_g, prm.nu, prm.DH)
    cnt = np.zeros_like(ux)
    cnt[:, 0, 0, 0] = N
    cnt[:, 1, 2, 1] = 3.0 * np.sin(2.0 * np.pi * 7.0 * t)  # a line at 7 Hz in one amplitude
    uy = np.zeros_like(ux)
    uy[:, 2, 1, 3] = 0.5
    fig = driver.mode_figures(prm, dict(step=np.arange(1, len(t) + 1), t=t, n=cnt, ux=ux, uy=uy, n_dropped=0))
    u_max = prm.gravity_g * prm.DH ** 2 / (8.0 * prm.nu)
    assert fig["U_max"] == u_max and fig["b"].shape == fig["b_exact"].shape == (len(t), ny + 1)
    assert np.max(np.abs(fig["b"] - fig["b_exact"])) <= 1e-15 * u_max
    assert np.array_equal(fig["tau_exact"][1:], prm.DH ** 2 / (prm.nu * n[1:] ** 2 * np.pi ** 2)) and np.isinf(fig["tau_exact"][0])
    for k in (1, 3, 5, 7):
        print(f"n = {k}: tau_fit / tau_exact - 1 = {fig['tau_fit'][k] / fig['tau_exact'][k] - 1.0:.3e}")
        assert abs(fig["tau_fit"][k] / fig["tau_exact"][k] - 1.0) <= 1e-9
    assert np.all(np.isnan(fig["tau_fit"][0::2]))
    assert fig["S"].shape == fig["E_uy"].shape == fig["f_peak"].shape == fig["f_box"].shape == (mx + 1, ny + 1)
    assert fig["S"][0, 0] == N and fig["S"][2, 2] == 0.0
    assert abs(fig["E_uy"][2, 1] * N * u_max ** 2 / 0.25 - 1.0) <= 1e-14 and fig["E_uy"][0, 0] == 0.0
    assert abs(fig["f_peak"][1, 2] - 7.0) <= fig["f_bin"] and np.isnan(fig["f_peak"][0, 0])
    c = prm.c_f * abs(prm.gravity_g * prm.DH ** 2 / (12.0 * prm.nu))
    assert fig["f_box"][0, 1] == c / (2.0 * prm.DH) and fig["f_box"][1, 0] == c / prm.DL and fig["f_box"][0, 0] == 0.0


def test_chunks_are_put_together_in_order(driver, capi):
    a = capi.modes_dict(np.array([[1.0, 0.1], [2.0, 0.2]]), np.arange(2 * 2 * 3 * 12, dtype=float).reshape(2, 2, 3, 3, 4))
    b = capi.modes_dict(np.array([[3.0, 0.3]]), -np.arange(2 * 3 * 12, dtype=float).reshape(1, 2, 3, 3, 4), n_dropped=0)
    out = driver._concat_modes([a, b])
    assert out["step"].tolist() == [1, 2, 3] and out["t"].tolist() == [0.1, 0.2, 0.3] and out["n_dropped"] == 0
    assert out["ux"].shape == (3, 2, 3, 4) and np.array_equal(out["ux"][:2], a["ux"]) and np.array_equal(out["ux"][2], b["ux"][0])
    assert a["n"][1, 1, 2, 3] == (((1 * 2 + 1) * 3 + 2) * 3 + 0) * 4 + 3  # record, m, n, field, basis: row-major
    err = driver._modes_lost("member 2: ", dict(a, n_dropped=5), 0.25, 2)
    assert "modes_capacity >= 7 (it is 2)" in str(err) and str(err).startswith("member 2: the mode amplitudes lost 5 records")


# 4 ---------------------------------------------------------------------------------------------------------------
def test_startup_distance_of_the_oracle(cfgmod, geom, profmod, oracle):
    """What the reference physics itself shows: the oracle's trajectory from rest, dp = 0.05, DL = 3, to t = 0.4, projected
    with profile.mode_sums after every step.  The largest distance of b_1 and b_3 from the closed form, in U_max, is
    mode_cases.STARTUP_DISTANCE -- the figure tests/test_gpu_modes.py holds the device's records to (x 1.5)."""
    s = mc.STARTUP
    prm = cfgmod.params_from_values(dp=s["dp"], DL=s["DL"], end_time=s["t_end"], output_interval=s["t_end"])
    parts = geom.init_particles(prm)
    t, pos, vel = mc.oracle_trajectory(oracle, prm, parts, s["t_end"])
    u_max = prm.gravity_g * prm.DH ** 2 / (8.0 * prm.nu)
    b = mc.b_series(profmod, prm, pos, vel)
    assert t[-1] == s["t_end"] and len(t) > 200
    for n, want in mc.STARTUP_DISTANCE.items():
        dist = float(np.max(np.abs(b[n] - profmod.mode_b_exact(n, t, prm.gravity_g, prm.nu, prm.DH)))) / u_max
        print(f"oracle, {len(t)} steps: b_{n} at most {dist:.5e} U_max from the closed form (b_{n}(0.4) = {b[n][-1] / u_max:.5f} U_max)")
        assert abs(dist / want - 1.0) <= 1e-4
