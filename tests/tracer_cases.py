"""Cases, id sets and comparisons shared by tests/test_tracers_host.py, tests/test_gpu_tracers.py, tests/test_gpu_batch_tracers.py
and tests/test_matlab_tracers.py (particle tracers, include/sphx.h sections 2p / 2q).

Every comparison of a record with the state is np.array_equal on the float64 arrays: k_tracers copies, so there is no
tolerance anywhere in these tests."""
import numpy as np

from probe_cases import CASES, case  # the samplers' small cases  # noqa: F401

FIELDS = ("x", "y", "u_x", "u_y")
SERIES = ("step", "t") + FIELDS
SMALL = ("dp05_auto", "dp025_walk", "dp05_dynamic", "dp025_dual", "two_cols", "one_col", "dp01_multi")
WAVE = 64  # lanes of a wave: one below, at and one above it are id-set sizes of their own


def id_sets(n_fluid, seed=5):
    """name -> ids: 1, 63, 64, 65, 300 (or all, where the channel holds fewer) and all n_fluid rows; shuffled, descending and
    ascending orders; rows 0 and n_fluid - 1 among them."""
    rng = np.random.default_rng(seed)
    ends = np.array([0, n_fluid - 1])

    def pick(n, order):
        n = min(n, n_fluid)
        rest = rng.choice(np.arange(1, n_fluid - 1), size=max(n - 2, 0), replace=False)
        ids = np.concatenate([ends, rest])[:n] if n >= 2 else np.array([n_fluid - 1])
        if order == "shuffled":
            ids = rng.permutation(ids)
        elif order == "descending":
            ids = np.sort(ids)[::-1]
        else:
            ids = np.sort(ids)
        return np.ascontiguousarray(ids, dtype=np.int64)

    return {"1": pick(1, "ascending"), "63": pick(WAVE - 1, "shuffled"), "64": pick(WAVE, "descending"), "65": pick(WAVE + 1, "ascending"),
            "300": pick(300, "shuffled"), "all": rng.permutation(n_fluid).astype(np.int64)}


def state_rows(profmod, state, ids):
    """profile.tracer_rows of a downloaded state: the definition"""
    return profmod.tracer_rows(state["pos"], state["vel"], ids)


def assert_record_is_state(tr, row, want, what):
    """record `row` of a tracers dict against the four [T] arrays of tracer_rows, bit for bit"""
    for k in FIELDS:
        assert tr[k][row].shape == want[k].shape, f"{what}: {k} {tr[k][row].shape} {want[k].shape}"
        assert np.array_equal(tr[k][row], want[k]), f"{what}: {k} differs in {int(np.count_nonzero(tr[k][row] != want[k]))} of {len(want[k])} columns"


def assert_series_identical(a, b, what):
    """two tracers dicts bit for bit, counters included"""
    assert np.array_equal(a["ids"], b["ids"]), what + ": ids"
    for k in SERIES:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), f"{what}: {k}"
    assert a["n_dropped"] == b["n_dropped"] and a["n_missing"] == b["n_missing"], what


def synthetic_series(x_true, y, u_x, t, DL, ids=None):
    """a tracers dict from unwrapped positions x_true [n, T]: x wrapped into [0, DL) as the state holds it"""
    x_true = np.asarray(x_true, dtype=np.float64)
    n, T = x_true.shape
    return dict(ids=np.arange(T, dtype=np.int32) if ids is None else np.asarray(ids, dtype=np.int32), step=np.arange(1, n + 1, dtype=np.int64),
                t=np.asarray(t, dtype=np.float64), x=x_true - np.floor(x_true / DL) * DL, y=np.broadcast_to(np.asarray(y, dtype=np.float64), (n, T)).copy(),
                u_x=np.broadcast_to(np.asarray(u_x, dtype=np.float64), (n, T)).copy(), u_y=np.zeros((n, T)), n_dropped=0, n_missing=0)
