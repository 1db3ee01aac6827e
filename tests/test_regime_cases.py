"""The regime cases do what they are for (not gpu): conditions on the INPUTS of tests/test_gpu_regimes.py and the switch
workers, established with the oracle and numpy alone (regime_cases.census), never with the library under test.

Measured with seed 7 (small: dp 0.05, DL 1.5, 600 fluid particles) and seed 31 (worker: dp 0.025, DL 1.5, 2 400), 35 steps,
`body` 12 steps; asserted are minima that leave room for another seed but not for a case that has stopped doing its job:

  case          size    pairs zero/linear/capped at the start -> capped at the end   limits     left/right crossings
  capped        small   2 873 / 2 262 / 604 of 5 739          -> 524                  V x 35     0 / 49
  capped        worker  11 897 / 11 496 / 269 of 23 662       -> 104                  V x 35     0 / 50
  left_capped   small   2 908 / 2 232 / 599                   -> 380                  A x 35     126 / 1
  left_capped   worker  11 836 / 11 560 / 266                 -> 531                  V x 35     130 / 1   rho/rho0 0.77..1.39
  leftward      small   0 capped                                                       A x 35     7 / 0
  leftward      worker  0 capped                                                       A x 35     17 / 0
  leftward_plain small / worker                                                        A x 35     11 / 0, 20 / 0
  viscous       small / worker                                                         V x 35     0 / 5, 0 / 0
  body          small   all 5 739 at du = 0                   -> 100                  BBBAAAAAAAAA   58 / 0   vmax 5.3
  body          worker  all 23 662 at du = 0                  -> 288                  BBAAAAAAAAAA   93 / 0
  floor         small / worker   rows 3 and 40 floored on step 1 (small: p = 0.41 and -0.37 after the step)
  default       small   0 capped, du_max 0.24 against c_f / 3 = 5                     A x 35     0 / 9
  default       worker  0 capped                                                       A x 35     0 / 21

The last two are the suite's own states: if they ever change, the assertions on them say what coverage moved."""
import numpy as np
import pytest

import regime_cases as rc

N_STEPS = 35
BODY_STEPS = 12
BUILDERS = dict(rc.CASES, default=rc.default, leftward_plain=rc.leftward_plain, viscous_plain=rc.viscous_plain)
_cache = {}


def _census(name, size, cfgmod, geom, oracle):
    if (name, size) not in _cache:
        prm, parts = BUILDERS[name](cfgmod, geom, size)
        _cache[name, size] = prm, parts, rc.census(prm, parts, oracle, BODY_STEPS if name == "body" else N_STEPS)
    return _cache[name, size]


@pytest.fixture(params=["small", "worker"])
def size(request):
    return request.param


def test_sizes_and_builders(size, cfgmod, geom):
    for name, build in BUILDERS.items():
        prm, parts = build(cfgmod, geom, size)
        assert parts["n_fluid"] == (600 if size == "small" else 2400), name
        assert prm.DL == 1.5 and prm.dp == (0.05 if size == "small" else 0.025), name
    assert set(rc.CASES) == {"leftward", "capped", "left_capped", "viscous", "body", "floor"}


def test_capped_has_every_pair_class(size, cfgmod, geom, oracle):
    prm, parts, c = _census("capped", size, cfgmod, geom, oracle)
    assert prm.c_f == 0.3
    for k in ("zero", "linear", "capped"):
        assert c["pairs_start"][k] >= 100, (k, c["pairs_start"])
    assert c["pairs_end"]["capped"] >= 100 and c["finite"]


def test_left_capped_crosses_leftward_with_capped_pairs(size, cfgmod, geom, oracle):
    prm, parts, c = _census("left_capped", size, cfgmod, geom, oracle)
    assert prm.gravity_g < 0 and prm.c_f == 0.3
    assert c["pairs_start"]["capped"] >= 100 and c["pairs_end"]["capped"] >= 100, (c["pairs_start"], c["pairs_end"])
    assert c["left"] >= 20 and c["finite"], c["left"]
    assert set(c["limits"]) <= set("AV") and len(c["limits"]) == N_STEPS
    assert 0.5 < c["rho_range"][0] and c["rho_range"][1] < 2.0
    assert np.all(parts["wall_vel"][parts["n_fluid"]:] != 0) and prm.rho0 == 2.5


@pytest.mark.parametrize("name", ["leftward", "leftward_plain"])
def test_leftward_crosses_the_seam_leftward_only(name, size, cfgmod, geom, oracle):
    prm, parts, c = _census(name, size, cfgmod, geom, oracle)
    nf = parts["n_fluid"]
    assert prm.gravity_g < 0 and np.all(parts["vel"][:nf, 0] < 0)
    assert c["left"] >= 5 and c["right"] == 0, (c["left"], c["right"])
    assert c["finite"]
    if name == "leftward":   # the mirror image of make_variant's walls
        top = parts["pos"][nf:, 1] > 0.5 * prm.DH
        assert np.all(parts["wall_vel"][nf:, 0][top] < 0) and np.all(parts["wall_vel"][nf:, 0][~top] > 0)


@pytest.mark.parametrize("name", ["viscous", "viscous_plain"])
def test_viscous_is_viscous_limited_on_every_step(name, size, cfgmod, geom, oracle):
    prm, parts, c = _census(name, size, cfgmod, geom, oracle)
    assert c["limits"] == "V" * N_STEPS, c["limits"]
    assert np.all(c["dt"] == rc.dt_viscous(prm)) and c["finite"]
    # what test_gpu_dual_rate.py needs refused: no room for two inner steps
    assert np.floor(min(rc.dt_viscous(prm), rc.dt_body(prm)) / (0.25 * prm.h / (prm.c_f + c["vmax"]))) < 2


def test_body_goes_from_body_limited_to_acoustic(size, cfgmod, geom, oracle):
    prm, parts, c = _census("body", size, cfgmod, geom, oracle)
    assert prm.gravity_g == -100.0 and not np.any(parts["vel"])
    assert c["limits"][0] == "B" and "A" in c["limits"] and set(c["limits"]) == set("AB"), c["limits"]
    assert c["dt"][0] == rc.dt_body(prm)
    assert c["left"] >= 20 and c["right"] == 0 and c["finite"], (c["left"], c["right"])
    assert c["pairs_start"]["zero"] == c["pairs_start"]["total"]    # at rest: every du is 0
    assert c["pairs_end"]["capped"] >= 50 and c["pairs_end"]["linear"] >= 100, c["pairs_end"]


def test_floor_rows_are_floored_on_the_first_step(size, cfgmod, geom, oracle):
    prm, parts, c = _census("floor", size, cfgmod, geom, oracle)
    assert c["floored"] == list(rc.FLOOR_ROWS)
    # without the floor the same rows would hold a large negative density: the floor decides their pressure
    one = oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=1, enable_sort=False)
    dt = one["stats"]["dt_last"]
    rows = list(rc.FLOOR_ROWS)
    assert np.all(np.abs(one["p"][rows]) < 0.01 * prm.p0)
    assert np.all(0.5 * dt * parts["drho_dt"][rows] < -10 * prm.rho0)


def test_the_suites_own_states_enter_none_of_it(size, cfgmod, geom, oracle):
    prm, parts, c = _census("default", size, cfgmod, geom, oracle)
    assert c["pairs_start"]["capped"] == 0 and c["pairs_end"]["capped"] == 0
    assert c["pairs_start"]["du_max"] < 0.1 * prm.c_f / 3.0
    assert c["limits"] == "A" * N_STEPS
    assert c["left"] == 0 and c["right"] >= 5
    assert c["floored"] == []
