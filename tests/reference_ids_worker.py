"""Child process of tests/test_reference_anchor.py::test_error_identifiers_equal_the_references: makes every malformed call of
MALFORMED against the reference's own MEX binaries (oracle/_ref/) and prints one JSON line per call, {"k": index} before the
call and {"k": index, "id": identifier or null} after it -- a call that the reference does not reject may crash this process,
and then the last line tells which one it was.

    python tests/reference_ids_worker.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

z, pairs = np.zeros(3), [np.ones(2)] * 6
P, N = "physics", "neighbor"
# (function, nargout or None for the mode's own, args): the malformed calls of test_host_logic.py::
# test_mex_surface_arity_and_shape_errors_need_no_device, test_gpu_mex_surface.py::test_error_ids and test_matlab_gateways.py
# that the reference rejects by an explicit check of its own (none of them had to be left out).
MALFORMED = [
    (P, None, ("density_correction",) + (z,) * 5), (P, None, ("viscous_force",) + (z,) * 3),
    (P, None, ("transport_correction",) + (z,) * 3), (P, None, ("integration_1st",)), (P, None, ("integration_2nd",)),
    (P, None, ("integration_verlet",)), (P, None, ("advance_shell_step",)), (P, None, ("wall_shear_monitor",)),
    (P, None, ("bogus",)), (P, None, ("no_such_mode",)), (P, 1, ()), (P, 1, (3.0,)), (P, None, ("density_correction", 1, 2, 3)),
    (P, 2, ("density_correction",) + (z,) * 13), (P, 4, ("integration_1st",) + (z,) * 21),
    (P, 8, ("advance_shell_step",) + (z,) * 23),
    (P, None, ("viscous_force", *pairs, np.zeros((4, 3)), np.zeros(4), np.zeros((4, 4)), 0.1, 0.1, 2, 4, np.ones(4), np.zeros((4, 2)))),
    (P, None, ("viscous_force", *pairs, np.zeros((4, 2)), np.zeros(5), np.zeros((4, 4)), 0.1, 0.1, 2, 4, np.ones(4), np.zeros((4, 2)))),
    (P, None, ("viscous_force", *pairs, np.zeros((4, 2)), np.zeros(4), np.zeros((4, 3)), 0.1, 0.1, 2, 4, np.ones(4), np.zeros((4, 2)))),
    (P, None, ("viscous_force", np.ones(2), np.ones(3), *([np.ones(2)] * 4), np.zeros((4, 2)), np.zeros(4), np.zeros((4, 4)), 0.1,
               0.1, 2, 4, np.ones(4), np.zeros((4, 2)))),
    (P, None, ("transport_correction", *pairs, np.zeros(4), np.zeros((4, 4)), np.zeros((4, 2)), 0.1, 2, 4, -1.0)),
    (P, None, ("transport_correction", *pairs, np.zeros(4), np.zeros((4, 4)), np.zeros((3, 2)), 0.1, 2, 4)),
    (P, None, ("density_correction", *pairs, np.ones(3), np.ones(4), 2, 4, 1.0, 0.1, 1.0)),
    (P, None, ("density_correction", *pairs, np.ones(2), np.ones(4), 0, 4, 1.0, 0.1, 1.0)),
    (P, None, ("density_correction", *pairs, np.ones(2), np.ones(5), 2, 4, 1.0, 0.1, 1.0)),
    (P, None, ("density_correction", *pairs, np.ones(2), np.ones(4), 2, 4, -1.0, 0.1, 1.0)),
    (P, None, ("density_correction", *pairs, np.ones(2), np.ones(4), 2, 4, 1.0, 0.0, 1.0)),
    (P, None, ("integration_2nd", *pairs, np.zeros(4), np.zeros(4), np.zeros((4, 2)), np.zeros((4, 1)), 0.1, 2, 4, np.zeros((4, 2)))),
    (P, None, ("integration_1st", *pairs, np.zeros(4), np.zeros((4, 4)), np.zeros(3), *([z] * 12))),
    (P, None, ("integration_verlet", *pairs, np.zeros(4), np.zeros((4, 4)), np.zeros(4), np.zeros(4), np.zeros((4, 2)),
               np.zeros((4, 2)), np.zeros(4), np.zeros((4, 2)), 0.1, 2, 4, 1.0, 0.0, 10.0, np.zeros((5, 2)))),
    (P, None, ("advance_shell_step", *pairs, np.ones(2), np.ones(4), np.zeros((4, 2)), np.zeros((4, 2)), np.zeros((4, 2)), np.ones(4),
               np.zeros(3), 0.1, 2, 4, *([1.0] * 7))),
    (P, None, ("wall_shear_monitor", *pairs, np.zeros((4, 2)), np.zeros((4, 2)), np.zeros((4, 2)), np.ones(4), np.zeros((4, 4)), 2,
               -1.0, 1.0, 0.1, 0.1)),
    (N, 7, (np.zeros((4, 3)), 2, 4, 0.1, 1.0)), (N, 7, (np.zeros((4, 2)), 2, 5, 0.1, 1.0)), (N, 7, (np.zeros((4, 2)), 5, 4, 0.1, 1.0)),
    (N, 7, (np.zeros((4, 2)), 0, 4, 0.1, 1.0)), (N, 7, (np.zeros((4, 2)), 2, 4, 0.1)), (N, 7, (np.zeros((4, 2)), 2, 4, 0.1, 1.0, 1.0)),
    (N, 7, (np.zeros((4, 2)), 2, 4, 0.1, -1.0)), (N, 7, (np.zeros((4, 2)), 2, 4, -0.1, 1.0)), (N, 6, (np.zeros((4, 2)), 2, 4, 0.1, 1.0)),
]


def call(surface, fn, nargout, args):
    f = surface.sph_physics_shell_mex if fn == P else surface.sph_neighbor_search_mex
    try:
        f(*args, **({} if nargout is None else {"nargout": nargout}))
    except surface.MexError as e:
        return e.identifier
    return None


def main():
    import mex_mock
    ref = mex_mock.reference_mex()
    if ref is None:
        print(json.dumps({"error": "no reference binaries"}), flush=True)
        return 2
    for k, (fn, nargout, args) in enumerate(MALFORMED):
        print(json.dumps({"k": k}), flush=True)
        print(json.dumps({"k": k, "id": call(ref, fn, nargout, args)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
