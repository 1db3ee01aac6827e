"""States shared by tests/test_field_map_host.py and tests/test_gpu_field_map.py."""
import numpy as np

from helpers import make_case


def void_case(cfgmod, geom):
    """dp 0.05, DL 3, jittered and developed: the fluid rows within 3h of (DL/2, DH/2) are left out of the arrays, so the
    nodes of a disc of radius about h around the centre have nobody within 2h."""
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.2, seed=9, developed=True)
    nf, nt = parts["n_fluid"], parts["n_total"]
    p = parts["pos"]
    keep = np.ones(nt, dtype=bool)
    keep[:nf] = np.hypot(p[:nf, 0] - 0.5 * prm.DL, p[:nf, 1] - 0.5 * prm.DH) >= 3.0 * prm.h
    out = {k: (np.asfortranarray(v[keep]) if isinstance(v, np.ndarray) and v.shape[:1] == (nt,) else v) for k, v in parts.items()}
    out["n_fluid"] = int(np.count_nonzero(keep[:nf]))
    out["n_total"] = int(np.count_nonzero(keep))
    return prm, out
