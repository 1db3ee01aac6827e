"""The dual-rate reference (tests/dual_rate_reference.py) checked on the CPU, before tests/test_gpu_dual_rate_parity.py relies
on it: it is the oracle's loop when n_in = 1, it tells four plausible mistakes of an inner sub-step from the right loop, its
result is well conditioned on every start the GPU cases use, those starts have the neighbour counts the GPU cases need, and
the clock clips the last outer step to the target.

Bounds.  Anchor: bitwise (the same C functions in the same order).  Telling apart: >= 1e-3 in max|a - b| / max|b| in some
field, seven decades above the bound the GPU cases assert.  Conditioning: a 1e-15 relative perturbation of the fluid's pos and
vel -- the size of one rounding -- may move no field by more than 1e-12 in that norm, two decades below the GPU bound of
1e-10: a start on which round-off grows faster would make that bound a statement about the start, not the kernels.
"""
import numpy as np
import pytest

import dual_rate_reference as drr

COMBOS = sorted({(c[0], c[2], c[3]) for k, c in drr.GPU_CASES.items() if k != "J"})


@pytest.fixture(scope="module")
def starts(cfgmod, geom, oracle):
    return {name: drr.start(cfgmod, geom, name) for name in ("plain", "bottom", "top", "seam", "variant", "left")}


@pytest.fixture(scope="module")
def right(starts):
    """drr.run on (start, n_in, outer steps), computed once per combination."""
    cache = {}

    def get(name, n_in, n_outer):
        key = (name, n_in, n_outer)
        if key not in cache:
            cache[key] = drr.run(*starts[name], n_in, max_outer=n_outer)
        return cache[key]
    return get


def test_substeps_reach_two_three_and_four(starts):
    prm, _ = starts["plain"]
    assert [drr.substeps(prm, d) for d in (0, 1, 2, 3, 4, 9)] == [1, 1, 2, 3, 4, 5]  # 5.36 acoustic steps fit
    prm, _ = starts["variant"]
    assert [drr.substeps(prm, d) for d in (2, 3, 4)] == [2, 3, 4]


@pytest.mark.parametrize("name", ["plain", "variant"])
def test_one_substep_is_the_oracles_loop_to_the_bit(name, starts, oracle):
    prm, parts = starts[name]
    got = drr.run(prm, parts, 1, max_outer=5)
    ref = oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=5, enable_sort=False)
    rs = ref["stats"]
    assert got["steps"] == 5 == rs["steps"]
    assert got["t"] == rs["t"] and got["dt_last"] == rs["dt_last"] and got["vmax"] == rs["vmax"]
    for k in drr.FIELDS:
        assert np.array_equal(got[k], ref[k]), k


def test_resuming_from_a_result_changes_nothing(starts, right):
    prm, parts = starts["plain"]
    first = drr.run(prm, parts, 2, max_outer=2)
    both = drr.run(prm, parts, 2, max_outer=3, state=first)
    whole = right("plain", 2, 10)
    more = drr.run(prm, parts, 2, max_outer=5, state=both)
    assert (first["steps"], both["steps"], more["steps"]) == (2, 5, 10)
    assert more["t"] == whole["t"] and more["dt_last"] == whole["dt_last"] and more["vmax"] == whole["vmax"]
    for k in drr.FIELDS:
        assert np.array_equal(more[k], whole[k]), k


@pytest.mark.parametrize("n_in,n_outer", [(2, 1), (3, 4)])
@pytest.mark.parametrize("wrong", drr.WRONG)
def test_a_wrong_inner_substep_shows(wrong, n_in, n_outer, starts, capsys):
    prm, parts = starts["plain"]
    ref = drr.run(prm, parts, n_in, max_outer=n_outer)
    bad = drr.run(prm, parts, n_in, max_outer=n_outer, wrong=wrong)
    err = drr.errors(bad, ref)
    with capsys.disabled():
        print(f"\n[dual-rate reference] {wrong}, n_in={n_in}, {n_outer} outer: "
              + " ".join(f"{k}={v:.1e}" for k, v in err.items()))
    assert max(err.values()) >= 1e-3, err


@pytest.mark.parametrize("name,n_in,n_outer", COMBOS, ids=[f"{a}-{b}x{c}" for a, b, c in COMBOS])
def test_every_gpu_start_is_well_conditioned(name, n_in, n_outer, starts, right, capsys):
    prm, parts = starts[name]
    nf = parts["n_fluid"]
    ref = right(name, n_in, n_outer)
    assert ref["steps"] == n_outer
    worst = 0.0
    for draw in range(3):
        rng = np.random.default_rng(1000 + draw)
        moved = dict(parts, pos=np.array(parts["pos"], order="F"), vel=np.array(parts["vel"], order="F"))
        for k in ("pos", "vel"):
            moved[k][:nf] *= 1.0 + 1e-15 * (rng.random((nf, 2)) * 2.0 - 1.0)
        assert not np.array_equal(moved["pos"], parts["pos"])
        got = drr.run(prm, moved, n_in, max_outer=n_outer)
        worst = max(worst, max(drr.errors(got, ref).values()), abs(got["dt_last"] - ref["dt_last"]) / ref["dt_last"],
                    abs(got["vmax"] - ref["vmax"]) / ref["vmax"])
    with capsys.disabled():
        print(f"\n[dual-rate reference] conditioning {name} n_in={n_in} {n_outer} outer: {worst:.1e}")
    assert worst <= 1e-12


def test_clipped_and_resumed_start_is_well_conditioned(starts):
    """Case J: advance to 2.5 first outer steps, then two more outer steps."""
    prm, parts = starts["plain"]
    nf = parts["n_fluid"]
    t1 = 2.5 * drr.first_outer_step(prm, parts, 2)

    def both(p):
        a = drr.run(prm, p, 2, t_target=t1)
        return a, drr.run(prm, p, 2, max_outer=2, state=a)
    ref = both(parts)
    assert (ref[0]["steps"], ref[1]["steps"]) == (3, 5)
    for draw in range(3):
        rng = np.random.default_rng(2000 + draw)
        moved = dict(parts, pos=np.array(parts["pos"], order="F"), vel=np.array(parts["vel"], order="F"))
        for k in ("pos", "vel"):
            moved[k][:nf] *= 1.0 + 1e-15 * (rng.random((nf, 2)) * 2.0 - 1.0)
        for got, r in zip(both(moved), ref):
            assert max(drr.errors(got, r).values()) <= 1e-12
            assert abs(got["dt_last"] - r["dt_last"]) <= 1e-12 * r["dt_last"]


def test_the_last_outer_step_is_clipped_to_the_target(starts):
    prm, parts = starts["plain"]
    for n_in in (2, 3):
        Dt = drr.first_outer_step(prm, parts, n_in)
        one = drr.run(prm, parts, n_in, max_outer=1)
        assert abs(one["t"] - Dt) <= 1e-15 and abs(one["dt_last"] - Dt / n_in) <= 1e-18
        got = drr.run(prm, parts, n_in, t_target=2.5 * Dt)
        assert got["steps"] == 3
        assert abs(got["t"] - 2.5 * Dt) <= 1e-12
        assert got["dt_last"] < 0.75 * one["dt_last"]  # about half an outer step was left
        again = drr.run(prm, parts, n_in, t_target=2.5 * Dt, state=got)  # at the target: nothing more to do
        assert again["steps"] == 3 and again["t"] == got["t"] and np.array_equal(again["pos"], got["pos"])
        capped = drr.run(prm, parts, n_in, t_target=1e9, t_end=2.5 * Dt)  # t_end clips like the target
        assert capped["steps"] == 3 and capped["t"] == got["t"] and np.array_equal(capped["vel"], got["vel"])


def test_four_substeps_on_the_squeezed_start_are_limited_by_advection(starts):
    """Case K: from the second outer step on max |v| exceeds c_f / (n_in - 1), so Dt = 0.25 h / max |v|."""
    prm, parts = starts["bottom"]
    start, n_in, n_outer = drr.GPU_CASES["K"][0], drr.GPU_CASES["K"][2], drr.GPU_CASES["K"][3]
    assert start == "bottom"
    st, limited = None, 0
    for _ in range(n_outer):
        vmax = drr._vmax(np.asarray((st or parts)["vel"]), parts["n_fluid"])
        st = drr.run(prm, parts, n_in, max_outer=1, state=st)
        if vmax * (n_in - 1) > prm.c_f:
            limited += 1
            assert abs(st["dt_last"] - 0.25 * prm.h / vmax / n_in) <= 1e-15
            assert st["dt_last"] < 0.75 * 0.25 * prm.h / (prm.c_f + vmax)
    assert limited >= 2


def test_plain_start_has_one_to_two_rows_of_sixteen(starts):
    prm, parts = starts["plain"]
    n_all, _ = drr.counts_within(prm, parts, 2.0 * prm.h)
    assert 16 < n_all.max() <= 32 and n_all.min() < 32


@pytest.mark.parametrize("name", ["bottom", "top", "seam"])
def test_squeezed_starts_have_wall_neighbours_behind_the_second_row(name, starts):
    prm, parts = starts[name]
    nf = parts["n_fluid"]
    n_all, n_wall = drr.counts_within(prm, parts, 2.0 * prm.h)
    crowded = n_all > 32
    assert crowded.any() and (crowded & (n_wall > 0)).any(), (n_all.max(), n_wall[crowded])
    x, y = parts["pos"][:nf, 0], parts["pos"][:nf, 1]
    assert np.all((x >= 0.0) & (x < prm.DL))
    near_wall = (y[crowded] > 0.5 * prm.DH) if name == "top" else (y[crowded] < 0.5 * prm.DH)
    assert near_wall.all()
    if name == "seam":  # crowded particles on both sides of x = 0
        assert (x[crowded] < 0.25 * prm.DL).any() and (x[crowded] > 0.75 * prm.DL).any()
    # the squeeze moved particles and nothing else; outside the circle the start is plain()'s
    p0 = starts["plain"][1]
    assert np.array_equal(parts["vel"], p0["vel"]) and np.array_equal(parts["pos"][nf:], p0["pos"][nf:])
    assert 0 < np.any(parts["pos"][:nf] != p0["pos"][:nf], axis=1).sum() < 80


def test_left_start_is_the_plain_one_mirrored_in_its_velocity(starts):
    (prm, parts), (prm0, p0) = starts["left"], starts["plain"]
    nf = parts["n_fluid"]
    assert prm.gravity_g == -prm0.gravity_g < 0 and np.array_equal(parts["pos"], p0["pos"])
    assert np.array_equal(parts["vel"], -p0["vel"]) and np.all(parts["vel"][:nf, 0] < 0)
    assert [drr.substeps(prm, d) for d in (2, 3, 4)] == [2, 3, 4]
    # ten outer steps of two cross the seam to the left (measured: one particle) and never to the right
    st, left, right = None, 0, 0
    for _ in range(drr.GPU_CASES["L"][3]):
        x0 = np.array((st or parts)["pos"][:nf, 0])
        st = drr.run(prm, parts, 2, max_outer=1, state=st)
        left += int(np.count_nonzero(st["pos"][:nf, 0] - x0 > 0.5 * prm.DL))
        right += int(np.count_nonzero(st["pos"][:nf, 0] - x0 < -0.5 * prm.DL))
    assert left >= 1 and right == 0, (left, right)
