"""The case table of tests/wall_rows_worker.py does what it is for, measured on the CPU with the oracle's neighbour search:
every case holds waves with a wall row next to waves without one, the higher channel holds more of the second kind, and the
dense case has lanes whose third or later row holds wall entries -- at 16 and at 32 lanes per particle, on the grid the device
reported when the fixtures were recorded (tests/golden/wall_rows_*.npz: cell columns, rows and skin)."""
import os

import numpy as np
import pytest

import wall_rows_worker as worker

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SINGLE = [c for c in worker.CASES if c != "batch4"]


def _census(case, lpp, cfgmod, geom, oracle, parts_of=lambda p: p):
    prm, parts, _ = worker.CASES[case](cfgmod, geom)
    parts = parts_of(parts)
    with np.load(os.path.join(GOLDEN, f"wall_rows_{case}_lpp{lpp}.npz")) as z:
        ncx, ncy, skin = int(z["n_cell_x"]), int(z["n_cell_y"]), float(z["skin"])
    nf, nt = parts["n_fluid"], parts["n_total"]
    nl = oracle.neighbor_search(parts["pos"], nf, nt, prm.h, prm.DL)
    return worker.census(nl[0], nl[1], parts["pos"], nf, lpp, prm.DL, ncx, ncy, float(np.min(parts["pos"][:, 1])),
                         2.0 * prm.h + skin)


@pytest.mark.parametrize("lpp", worker.LANES)
@pytest.mark.parametrize("case", SINGLE)
def test_every_case_holds_the_waves_it_is_for(case, lpp, cfgmod, geom, oracle):
    c = _census(case, lpp, cfgmod, geom, oracle)
    print(f"{case} at {lpp} lanes: {c}")
    worker.check_census(case, c)
    n_fluid = worker.CASES[case](cfgmod, geom)[1]["n_fluid"]
    assert c["waves"] == -(-n_fluid // (64 // lpp)) and 0 < c["wall_particles"] < n_fluid, c


@pytest.mark.parametrize("lpp", worker.LANES)
def test_batch_members_are_the_first_case_at_four_seeds(lpp, cfgmod, geom, oracle):
    prm, members, _ = worker.CASES["batch4"](cfgmod, geom)
    _, first, _ = worker.CASES["slots_developed"](cfgmod, geom)
    assert len(members) == worker.MEMBERS
    assert np.array_equal(members[0]["pos"], first["pos"]) and np.array_equal(members[0]["vel"], first["vel"])
    for k, m in enumerate(members[1:], 1):
        assert not np.array_equal(m["pos"], first["pos"]), k
        assert np.array_equal(m["mass"], first["mass"]) and np.array_equal(m["wall_vel"], first["wall_vel"]), k
    c = _census("batch4", lpp, cfgmod, geom, oracle, parts_of=lambda ms: ms[worker.MEMBERS - 1])
    assert c["wall_waves"] > 0 and c["interior_waves"] > 0, c


def test_the_table_names_every_case_once():
    named = set(worker.BOTH_CLASSES) | {"batch4"}
    assert named == set(worker.CASES)
    assert set(worker.INTERIOR_MAJORITY) | set(worker.THIRD_WALL_ROW) <= set(worker.BOTH_CLASSES)
