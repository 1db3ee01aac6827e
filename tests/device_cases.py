"""Inputs and exact references for the unit tests of the device functions (tests/test_gpu_device_formulas.py,
tests/test_gpu_device_index.py; checked themselves, without a GPU, by tests/test_device_cases.py).

Every function of csrc/sphx_device.hpp and the helpers of sphx_kernels.hpp / sphx_flow_stats.hpp / sphx_pair_dist.hpp /
sphx_grad_stats.hpp gets: seeded random inputs, hand-placed edges, an EXACT reference on those double inputs (rational
arithmetic, fractions.Fraction; mpmath at 50 digits where a square root comes in; plain Python / numpy for the integer and
edge-deciding functions) and, for the floating-point formulas, a plain numpy evaluation of the same expression in double, in
the header's operation order and without fused multiply-adds -- the baseline a device error is allowed against.

Nothing here calls the library under test.  eps = 2^-52 throughout ("ulp" of a relative error: one eps)."""
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np

EPS = 2.0 ** -52
DP_ALL = (0.002, 0.004, 0.005, 0.01, 0.0125, 0.02, 0.025, 0.04, 0.05, 0.1)
DP_BASELINE = (0.05, 0.025, 0.01, 0.002)
N_RANDOM = 4000
na = np.nextafter
mpmath.mp.dps = 50


def h_of(dp):
    return 1.3 * dp  # config.params_from_values


def kernel_const(h):
    """make_kernel_const (sphx_device.hpp), operation by operation: (h, inv_h, sigma, sigma_over_h, rcut2)."""
    h = float(h)
    sigma = 10.0 / (7.0 * np.pi * h * h)
    return (h, 1.0 / h, sigma, sigma / h, (2.0 * h) * (2.0 * h))


def F(x):
    return Fraction(float(x))


def frac_err(values, exact):
    """|value - exact| per element, as doubles (the subtraction is exact, only the result is rounded)."""
    return np.array([float(abs(Fraction(float(v)) - e)) for v, e in zip(values, exact)])


def ulp(x):
    return float(np.spacing(np.abs(np.float64(x))))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------------------------
# A. per-pair arithmetic
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def rcp_inputs():
    """x for rcp_nr: log-uniform over 1e-12 .. 1e12, powers of two, the h of every dp."""
    rng = np.random.default_rng(101)
    x = 10.0 ** rng.uniform(-12.0, 12.0, N_RANDOM)
    return np.concatenate([x, 2.0 ** np.arange(-40, 41), [h_of(dp) for dp in DP_ALL]])


@functools.lru_cache(None)
def rsqrt_inputs():
    """x for rsqrt_nr (squared pair distances, 1e-24 < x): log-uniform over (1e-24, 1e12], the first double above 1e-24, 4 h^2 of
    every h, even and odd powers of two, 1e300."""
    rng = np.random.default_rng(102)
    x = 10.0 ** rng.uniform(-24.0, 12.0, N_RANDOM)
    x = x[x > 1e-24]
    hs = [(2.0 * h_of(dp)) * (2.0 * h_of(dp)) for dp in DP_ALL]
    return np.concatenate([x, [na(1e-24, 1.0)], hs, 2.0 ** np.arange(-78, 41), [1e300]])


OUT_OF_DOMAIN = np.array([0.0, 5e-324, 1e-310, np.inf])  # printed by the GPU tests, not asserted


def rcp_rel_error(x, y):
    """(x y - 1) exactly: the relative error of y as 1 / x, to first order -- in eps."""
    return np.array([float(F(a) * F(b) - 1) for a, b in zip(x, y)]) / EPS


def rsqrt_rel_error(x, y):
    """The relative error d of y as 1 / sqrt(x), from the exact residual x y^2 - 1 = 2 d + d^2 -- in eps."""
    res = np.array([float(F(a) * F(b) * F(b) - 1) for a, b in zip(x, y)])
    return (np.sqrt(1.0 + res) - 1.0 if np.max(np.abs(res)) > 1e-6 else 0.5 * res) / EPS


def np_rsqrt(x):
    return 1.0 / np.sqrt(x)


@functools.lru_cache(None)
def pair_geom_inputs():
    """(dx, dy): random pairs inside the support of the baseline h, pairs at the kR2Min filter (r^2 just above 1e-24),
    axis-aligned pairs of either sign, |dx| >> |dy| and the reverse."""
    rng = np.random.default_rng(103)
    dx, dy = [], []
    for dp in DP_BASELINE:
        r = rng.uniform(0.0, 2.0 * h_of(dp), N_RANDOM // 4)
        a = rng.uniform(0.0, 2.0 * np.pi, r.size)
        dx.append(r * np.cos(a)); dy.append(r * np.sin(a))
    t = na(1e-12, 1.0)
    edge_x = [t, 0.0, -t, 8e-13, 1e-12, 0.13, -0.13, 0.0, 0.0, 0.1, 1e-9, 0.13, 3e-17, 2.0 ** -20, 1.0]
    edge_y = [0.0, t, 0.0, 6.1e-13, 1e-13, 0.0, 0.0, 0.065, -0.065, 1e-13, 0.1, 1e-17, 0.13, 2.0 ** -20, 1.0]
    dx.append(np.array(edge_x)); dy.append(np.array(edge_y))
    dx, dy = np.concatenate(dx), np.concatenate(dy)
    keep = dx * dx + dy * dy > 1e-24  # the neighbour filter (kR2Min): nothing else reaches pair_geom
    return dx[keep], dy[keep]


def exact_r(dx, dy):
    """sqrt(dx^2 + dy^2) at 50 digits."""
    return [mpmath.sqrt(mpmath.mpf(float(a)) ** 2 + mpmath.mpf(float(b)) ** 2) for a, b in zip(dx, dy)]


def mp_rel_err(values, exact):
    return np.array([float(abs(mpmath.mpf(float(v)) - e) / abs(e)) for v, e in zip(values, exact)])


# pair_geom: r2 = dx dx + dy dy carries at most 1 eps (two products and a sum, or a product and a fused multiply-add), so its
# root 0.5 eps; inv_r at most the 2 eps asserted for rsqrt_nr; the product r2 * inv_r another 0.5 eps
PAIR_GEOM_R_BOUND = 0.5 + 2.0 + 0.5  # eps, relative
PAIR_GEOM_UNIT_BOUND = 4.0           # eps: |ex^2 + ey^2 - 1|


def unit_defect(ex, ey):
    return np.array([float(F(a) * F(a) + F(b) * F(b) - 1) for a, b in zip(ex, ey)]) / EPS


def r_for_q(q, h, inv_h):
    """A double r with fl(r * inv_h) == q, or the nearest thing to it (searched a few ulps around q * h)."""
    r = q * h
    cands = [r]
    lo = hi = r
    for _ in range(6):
        lo, hi = na(lo, -np.inf), na(hi, np.inf)
        cands += [lo, hi]
    cands.sort(key=lambda c: (abs(c * inv_h - q), abs(c - r)))
    return cands[0]


SPLINE_FORMS = ("spline", "spline_dW", "spline_W", "spline_dW_sel", "spline_dW_in", "spline_W_sel")


@functools.lru_cache(None)
def spline_inputs(dp):
    """r = q h inside the support, for the six spellings of the cubic spline: q random in [0, 2); q = 1 exactly and one ulp
    either side; 1 +- 1e-6 U; 2 - 1e-6 U; the last double below 2 h; q <= 1e-6.  -> dict(kc, r, near1: mask of the inputs
    within 1e-5 of q = 1)."""
    h = h_of(dp)
    kc = kernel_const(h)
    rng = np.random.default_rng(int(round(dp * 1e6)))
    q = rng.uniform(0.0, 2.0, N_RANDOM)
    r = [q * h]
    r.append(np.array([r_for_q(t, h, kc[1]) for t in (1.0, na(1.0, 0.0), na(1.0, 2.0))]))
    u = rng.uniform(0.0, 1.0, 64)
    r.append((1.0 + 1e-6 * u) * h); r.append((1.0 - 1e-6 * u) * h)
    r.append((2.0 - 1e-6 * u) * h)
    r.append(np.array([na(2.0 * h, 0.0)]))
    r.append(np.concatenate([1e-6 * rng.uniform(0.0, 1.0, 32) * h, [0.0, 1e-300]]))
    r = np.concatenate(r)
    assert np.all(r < 2.0 * h)
    return dict(h=h, kc=kc, r=r, near1=np.abs(r * kc[1] - 1.0) < 1e-5)


def beyond_support(dp):
    """r just outside 2 h: the next double and a few ulps beyond (preconditions of spline_dW_in / spline_W_sel)."""
    h = h_of(dp)
    r, out = 2.0 * h, []
    for _ in range(4):
        r = na(r, np.inf)
        out.append(r)
    return np.array(out)


def outside_q(dp):
    """r at q = 2, 2 + ulp, 3, 1e6: spline_dW_sel returns zero there.  q is the EXACT product r * inv_h: the compiler fuses
    2 - r * inv_h into one multiply-add, so the device never rounds q, and an r whose product rounds to 2.0 from below is still
    inside the support (a = 1e-16, W' = -0.75 sigma/h 1e-32: the true value, and what the exact reference gives too).  So each r is
    the first double whose exact product reaches the target (for some h no product lies in [2, 2 + ulp / 2): the first one then rounds
    to the double after 2.0)."""
    h = h_of(dp)
    kc = kernel_const(h)
    out = []
    for t in (2.0, na(2.0, 3.0), 3.0, 1e6):
        r = r_for_q(t, h, kc[1])
        while F(r) * F(kc[1]) >= F(t):
            r = na(r, 0.0)
        while F(r) * F(kc[1]) < F(t):
            r = na(r, np.inf)
        out.append(r)
    return np.array(out)


def spline_exact(kc, r):
    """(W, dW) of the cubic spline on the double inputs, exactly: q = r * inv_h as a rational number, the two-piece polynomial,
    times the double sigma resp. sigma_over_h."""
    _, inv_h, sigma, soh, _ = (F(v) for v in kc)
    W, dW = [], []
    for x in r:
        q = F(x) * inv_h
        if q < 1:
            W.append(sigma * (1 - Fraction(3, 2) * q * q + Fraction(3, 4) * q * q * q))
            dW.append(soh * (-3 * q + Fraction(9, 4) * q * q))
        elif q < 2:
            t = 2 - q
            W.append(sigma * Fraction(1, 4) * t * t * t)
            dW.append(-soh * Fraction(3, 4) * t * t)
        else:
            W.append(Fraction(0)); dW.append(Fraction(0))
    return W, dW


def spline_numpy(kc, r, form):
    """The header's expression of `form` in numpy double, in its operation order, no fused multiply-add -> (W, dW); None for
    the one the form does not give."""
    _, inv_h, sigma, soh, _ = kc
    q = r * inv_h
    W = dW = None
    if form in ("spline", "spline_dW", "spline_W"):
        tq = 2.0 - q
        inner, outer = q < 1.0, (q >= 1.0) & (q < 2.0)
        if form != "spline_dW":
            W = np.where(inner, sigma * (1.0 - 1.5 * q * q + 0.75 * q * q * q), np.where(outer, sigma * 0.25 * tq * tq * tq, 0.0))
        if form != "spline_W":
            dW = np.where(inner, soh * (-3.0 * q + 2.25 * q * q), np.where(outer, -soh * 0.75 * tq * tq, 0.0))
    else:
        a = np.maximum(2.0 - q, 0.0) if form == "spline_dW_sel" else 2.0 - q
        b = np.maximum(1.0 - q, 0.0)
        if form == "spline_W_sel":
            W = (0.25 * sigma) * ((-4.0 * (b * b)) * b + (a * a) * a)
        else:
            dW = (-0.75 * soh) * ((-4.0 * b) * b + a * a)
    return W, dW


# the recorded worst errors of the numpy-double evaluations over spline_inputs(dp), dp in DP_BASELINE, in eps of the scale
# (sigma for W, sigma / h for dW); tests/test_device_cases.py asserts them with a factor 1.25 of slack
BASELINE = dict(W_two_piece=1.8, dW_two_piece=3.8, W_branch_free=3.3, dW_branch_free=3.6, rsqrt=0.75)


@functools.lru_cache(None)
def spline_reference(dp):
    """-> dict: exact W / dW (Fractions), and per form the numpy-double errors in eps of the scale (W_err, dW_err arrays)."""
    c = spline_inputs(dp)
    kc, r = c["kc"], c["r"]
    W, dW = spline_exact(kc, r)
    out = dict(W=W, dW=dW, np_err={})
    for form in SPLINE_FORMS:
        Wn, dWn = spline_numpy(kc, r, form)
        out["np_err"][form] = (None if Wn is None else frac_err(Wn, W) / (EPS * kc[2]),
                               None if dWn is None else frac_err(dWn, dW) / (EPS * kc[3]))
    return out


def spline_bound(np_worst):
    """Allowed |device - exact| in eps of the scale: twice the worst numpy-double error of the same form over the same inputs,
    plus 2 eps (fused multiply-adds round differently; q itself is rounded)."""
    return 2.0 * np_worst + 2.0


# ---- per-pair terms: one pair at a time, accumulated into zeros ----
@functools.lru_cache(None)
def pair_term_inputs():
    """Pairs inside the support of dp = 0.05 with volumes, velocities, a B matrix, an acceleration, a pressure and a density:
    columns by name.  The first rows are hand-placed: a separating and an approaching pair along x, and three wall pairs
    whose `face` = -(a . e) is negative, zero and positive."""
    rng = np.random.default_rng(104)
    dp = 0.05
    h = h_of(dp)
    n = 1000
    r = rng.uniform(0.05 * h, 1.999 * h, n)
    a = rng.uniform(0.0, 2.0 * np.pi, n)
    c = dict(dx=r * np.cos(a), dy=r * np.sin(a), vol=dp * dp * rng.uniform(0.8, 1.2, n),
             vxi=rng.uniform(-1.5, 1.5, n), vyi=rng.uniform(-0.2, 0.2, n), ujx=rng.uniform(-1.5, 1.5, n), ujy=rng.uniform(-0.2, 0.2, n),
             b11=rng.uniform(0.9, 1.6, n), b12=rng.uniform(-0.2, 0.2, n), b21=rng.uniform(-0.2, 0.2, n), b22=rng.uniform(0.9, 2.0, n),
             acx=rng.uniform(-1.0, 1.0, n), acy=rng.uniform(-1.0, 1.0, n), p=rng.uniform(-5.0, 50.0, n), rhoh=rng.uniform(0.95, 1.05, n))
    # i at the origin side: dx = x_i - x_j > 0, e = +x.  separating: v_i - u_j along +e; approaching: along -e
    for k, (vxi, ujx) in enumerate(((1.0, 0.25), (0.25, 1.0))):
        c["dx"][k], c["dy"][k], c["vxi"][k], c["ujx"][k], c["vyi"][k], c["ujy"][k] = 0.06, 0.0, vxi, ujx, 0.0, 0.0
    # wall pairs straight below the particle (e = +y): face = -acy
    for k, acy in ((2, 1.0), (3, 0.0), (4, -1.0)):
        c["dx"][k], c["dy"][k], c["acx"][k], c["acy"][k] = 0.0, 0.04, 0.3, acy
    return dict(h=h, kc=kernel_const(h), n=n, **c)


def _dW_in_mp(kc, r):
    """spline_dW_in's polynomial at an mpmath r (inside the support)."""
    inv_h, soh = mpmath.mpf(kc[1]), mpmath.mpf(kc[3])
    q = r * inv_h
    a, b = 2 - q, (1 - q if q < 1 else mpmath.mpf(0))
    return mpmath.mpf("-0.75") * soh * (a * a - 4 * b * b)


@functools.lru_cache(None)
def pair_term_reference():
    """-> per term: (names of the input columns, exact outputs [n][k] as doubles rounded from 50 digits, numpy-double outputs
    [n][k], scale [n] the errors are measured in)."""
    c = pair_term_inputs()
    kc, n = c["kc"], c["n"]
    M = mpmath.mpf
    ex_out = {k: [] for k in ("kgc_moment_add", "continuity_add", "wall_pair", "wall_pressure_add")}
    for i in range(n):
        v = {k: M(float(c[k][i])) for k in c if isinstance(c[k], np.ndarray)}
        r = mpmath.sqrt(v["dx"] ** 2 + v["dy"] ** 2)
        ex, ey = v["dx"] / r, v["dy"] / r
        dW = _dW_in_mp(kc, r)  # (inside the support all spellings are the same polynomial)
        f = dW * v["vol"]
        ex_out["kgc_moment_add"].append([-v["dx"] * f * ex, -v["dx"] * f * ey, -v["dy"] * f * ex, -v["dy"] * f * ey])
        ex_out["continuity_add"].append([((v["vxi"] - v["ujx"]) * ex + (v["vyi"] - v["ujy"]) * ey) * f])
        tx, ty = v["b11"] * ex + v["b12"] * ey, v["b21"] * ex + v["b22"] * ey
        ex_out["wall_pair"].append([r, f, tx, ty, ex * tx + ey * ty])
        face = -(v["acx"] * ex + v["acy"] * ey)
        p_wall = v["p"] + v["rhoh"] * r * (face if face > 0 else 0)
        ex_out["wall_pressure_add"].append([-(v["p"] + p_wall) * f * tx, -(v["p"] + p_wall) * f * ty])
    # numpy double, the header's order: pair_geom with a correctly rounded 1 / sqrt
    dx, dy, vol = c["dx"], c["dy"], c["vol"]
    r2 = dx * dx + dy * dy
    inv_r = np_rsqrt(r2)
    r = r2 * inv_r
    ex, ey = dx * inv_r, dy * inv_r
    dW = spline_numpy(kc, r, "spline_dW_in")[1]
    f = dW * vol
    tx, ty = c["b11"] * ex + c["b12"] * ey, c["b21"] * ex + c["b22"] * ey
    face = -(c["acx"] * ex + c["acy"] * ey)
    p_wall = c["p"] + c["rhoh"] * r * np.maximum(0.0, face)
    np_out = dict(
        kgc_moment_add=np.stack([0.0 - dx * (f * ex), 0.0 - dx * (f * ey), 0.0 - dy * (f * ex), 0.0 - dy * (f * ey)], 1),
        continuity_add=np.stack([0.0 + ((c["vxi"] - c["ujx"]) * ex + (c["vyi"] - c["ujy"]) * ey) * spline_numpy(kc, r, "spline_dW_sel")[1] * vol], 1),
        wall_pair=np.stack([r, f, tx, ty, ex * tx + ey * ty], 1),
        wall_pressure_add=np.stack([0.0 - (c["p"] + p_wall) * f * tx, 0.0 - (c["p"] + p_wall) * f * ty], 1))
    # scales: the size of the largest product a term is made of
    soh_vol = kc[3] * vol
    bmax = np.abs(c["b11"]) + np.abs(c["b12"]) + np.abs(c["b21"]) + np.abs(c["b22"])
    scale = dict(kgc_moment_add=np.stack([soh_vol * np.hypot(dx, dy)] * 4, 1),
                 continuity_add=np.stack([soh_vol * (np.abs(c["vxi"] - c["ujx"]) + np.abs(c["vyi"] - c["ujy"]))], 1),
                 wall_pair=np.stack([r, soh_vol, bmax, bmax, bmax], 1),
                 wall_pressure_add=np.stack([soh_vol * bmax * (2.0 * np.abs(c["p"]) + c["rhoh"] * r * np.hypot(c["acx"], c["acy"]))] * 2, 1))
    cols = dict(kgc_moment_add=("dx", "dy", "vol"), continuity_add=("dx", "dy", "vxi", "vyi", "ujx", "ujy", "vol"),
                wall_pair=("dx", "dy", "vol", "b11", "b12", "b21", "b22"),
                wall_pressure_add=("dx", "dy", "vol", "b11", "b12", "b21", "b22", "acx", "acy", "p", "rhoh"))
    out = {}
    for k in ex_out:
        exact = ex_out[k]
        np_err = np.array([[float(abs(M(float(np_out[k][i, j])) - exact[i][j])) for j in range(len(exact[i]))] for i in range(n)])
        out[k] = dict(cols=cols[k], exact=exact, np_err=np_err / (EPS * scale[k]), scale=scale[k])
    return out


def mp_err(values, exact):
    """|values[i][j] - exact[i][j]| for exact mpmath numbers -> array."""
    return np.array([[float(abs(mpmath.mpf(float(values[i][j])) - exact[i][j])) for j in range(len(exact[i]))] for i in range(len(exact))])


# ---- kgc_from_A ----
def kgc_exact(a11, a12, a21, a22):
    """kgc_from_A in rational arithmetic (sphx_device.hpp; the thresholds are the reference's)."""
    a11, a12, a21, a22 = F(a11), F(a12), F(a21), F(a22)
    reg = F(1e-8)
    n11, n12, n22 = a11 * a11 + a21 * a21 + reg, a11 * a12 + a21 * a22, a12 * a12 + a22 * a22 + reg
    det_n = n11 * n22 - n12 * n12
    P = [Fraction(1), Fraction(0), Fraction(0), Fraction(1)]
    if not abs(det_n) < F(1e-20):
        i11, i12, i22 = n22 / det_n, -n12 / det_n, n11 / det_n
        P = [i11 * a11 + i12 * a12, i11 * a21 + i12 * a22, i12 * a11 + i22 * a12, i12 * a21 + i22 * a22]
    det_a = a11 * a22 - a12 * a21
    deficit = max(1 - det_a, Fraction(0))
    total = det_a + deficit
    lam, rest = Fraction(0), Fraction(1)
    if not abs(total) < F(1e-12):
        lam, rest = det_a / total, deficit / total
    return [lam * P[0] + rest, lam * P[1], lam * P[2], lam * P[3] + rest]


def kgc_numpy(a11, a12, a21, a22):
    """The same in numpy double (arrays), in the header's order."""
    n11 = a11 * a11 + a21 * a21 + 1e-8
    n12 = a11 * a12 + a21 * a22
    n22 = a12 * a12 + a22 * a22 + 1e-8
    det_n = n11 * n22 - n12 * n12
    sing = np.abs(det_n) < 1e-20
    dn = np.where(sing, 1.0, det_n)
    i11, i12, i22 = n22 / dn, -n12 / dn, n11 / dn
    P = [np.where(sing, 1.0, i11 * a11 + i12 * a12), np.where(sing, 0.0, i11 * a21 + i12 * a22),
         np.where(sing, 0.0, i12 * a11 + i22 * a12), np.where(sing, 1.0, i12 * a21 + i22 * a22)]
    det_a = a11 * a22 - a12 * a21
    deficit = np.maximum(1.0 - det_a, 0.0)
    total = det_a + deficit
    none = np.abs(total) < 1e-12
    tt = np.where(none, 1.0, total)
    lam, rest = np.where(none, 0.0, det_a / tt), np.where(none, 1.0, deficit / tt)
    return np.stack([lam * P[0] + rest, lam * P[1], lam * P[2], lam * P[3] + rest], 1)


KGC_NAMED = dict(
    identity=(1.0, 0.0, 0.0, 1.0),
    zero=(0.0, 0.0, 0.0, 0.0),                       # B = I exactly
    wall_truncated=(0.98, 0.01, -0.02, 0.5),         # a particle next to a wall: half its support in y is missing
    det_just_below_1=(1.0, 0.0, 0.0, na(1.0, 0.0)),  # deficit = 2^-53
    det_just_above_1=(1.0, 0.0, 0.0, na(1.0, 2.0)),  # deficit = 0
    det_above_1=(1.05, 0.02, 0.01, 1.1),
    det_negative=(0.3, 0.9, 0.8, 0.2),
    det_negative_large=(-1.0, 0.2, 0.1, 1.3),
)
# rank one: det A = 0, so lambda = 0 and B = I, whatever the regularised P is (its entries are of order 1 / |A| here, below 200:
# a det A that a fused multiply-add leaves at 1e-17 |A|^2 instead of 0 moves B by less than 1e-15).  A group of its own.
KGC_RANK_ONE = ((1.0, 0.5, 2.0, 1.0), (0.3, 0.3, 0.3, 0.3), (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.7, 0.0), (0.5, -0.25, -1.0, 0.5),
                (1e-3, 2e-3, 2e-3, 4e-3))


@functools.lru_cache(None)
def kgc_cases():
    """-> dict(A [n][4], group [n] (0: named + random, 1: rank one), names, exact [n][4] Fractions, np_err [n] -- the largest
    entry error of the numpy-double evaluation relative to max(1, max |B|))."""
    rng = np.random.default_rng(105)
    A = [list(v) for v in KGC_NAMED.values()]
    while len(A) < len(KGC_NAMED) + 1000:  # moment matrices of complete and of truncated supports
        m = [rng.uniform(0.45, 1.15), rng.uniform(-0.15, 0.15), rng.uniform(-0.15, 0.15), rng.uniform(0.45, 1.15)]
        if 0.2 <= m[0] * m[3] - m[1] * m[2] <= 1.2:
            A.append(m)
    group = [0] * len(A) + [1] * len(KGC_RANK_ONE)
    A = np.array(A + [list(v) for v in KGC_RANK_ONE])
    exact = [kgc_exact(*row) for row in A]
    scale = np.array([max(1.0, max(abs(float(e)) for e in row)) for row in exact])
    B = kgc_numpy(*A.T)
    return dict(A=A, group=np.array(group), names=list(KGC_NAMED), exact=exact, scale=scale, np_err=kgc_err(B, exact, scale))


def kgc_err(B, exact, scale):
    return np.array([max(float(abs(F(B[i][j]) - exact[i][j])) for j in range(4)) for i in range(len(exact))]) / scale


def kgc_bound(np_worst):
    return 4.0 * np_worst + 1e-15


# ---- small per-particle formulas ----
def riemann_numpy(ul, ur, cf):
    """fmin(3 max(ul - ur, 0), c_f) as the reference states it (`if (x < 0) x = 0`: a -0.0 stays -0.0, which numpy's maximum
    leaves open)."""
    a = ul - ur
    a = np.where(a < 0.0, 0.0, a)
    return np.fmin(3.0 * a, cf)


@functools.lru_cache(None)
def riemann_inputs():
    rng = np.random.default_rng(106)
    cf = 15.0
    ul, ur = rng.uniform(-8.0, 8.0, N_RANDOM), rng.uniform(-8.0, 8.0, N_RANDOM)
    edge_l = [5.0, 1.25, -0.0, 0.0, 0.0, 7.0, na(5.0, 9.0), na(5.0, 0.0), -3.0, 2.0]
    edge_r = [0.0, 1.25, 0.0, -0.0, 0.0, 1.0, 0.0, 0.0, 2.0, -3.0]  # ul - ur = c_f / 3 = 5 in the first; equal speeds; -0.0
    return np.concatenate([ul, edge_l]), np.concatenate([ur, edge_r]), np.full(N_RANDOM + len(edge_l), cf)


@functools.lru_cache(None)
def transport_cases():
    """inc, h, coeff: random on both sides of the fade, fade exactly 1 (100 |inc|^2 = h^2), one ulp either side, inc = 0.
    -> dict(inc_x, inc_y, h, coeff, exact [n][2], np [n][2], fade_exact [n])."""
    rng = np.random.default_rng(107)
    h = h_of(0.05)
    mag = 10.0 ** rng.uniform(-4.0, 0.0, N_RANDOM) * h  # the fade reaches 1 at |inc| = h / 10
    a = rng.uniform(0.0, 2.0 * np.pi, N_RANDOM)
    ix, iy = mag * np.cos(a), mag * np.sin(a)
    # fade == 1 exactly needs 100 (ix^2 + iy^2) == h^2 in doubles: inc = (2^-k, 0), h = 10 * 2^-k -> 100 * 2^-2k = h^2
    e = 2.0 ** -7
    hx = 10.0 * e
    edge = [(e, 0.0, hx), (0.0, e, hx), (na(e, 0.0), 0.0, hx), (na(e, 1.0), 0.0, hx), (0.0, 0.0, hx), (-e, 0.0, hx), (0.0, -0.0, h)]
    ix = np.concatenate([ix, [v[0] for v in edge]]); iy = np.concatenate([iy, [v[1] for v in edge]])
    hh = np.concatenate([np.full(N_RANDOM, h), [v[2] for v in edge]])
    coeff = np.concatenate([rng.uniform(0.05, 0.5, N_RANDOM), np.full(len(edge), 0.2)])
    exact, fades = [], []
    for x, y, H, c in zip(ix, iy, hh, coeff):
        x, y, H, c = F(x), F(y), F(H), F(c)
        fade = min(max(100 * (x * x + y * y) / (H * H), Fraction(0)), Fraction(1))
        fades.append(fade)
        exact.append([c * H * H * fade * x, c * H * H * fade * y])
    fade = 100.0 * (ix * ix + iy * iy) / (hh * hh)
    gain = coeff * hh * hh
    fade = np.where(fade > 1.0, 1.0, fade)
    fade = np.where(fade < 0.0, 0.0, fade)
    return dict(inc_x=ix, inc_y=iy, h=hh, coeff=coeff, exact=exact, fade_exact=fades, np=np.stack([gain * fade * ix, gain * fade * iy], 1))


@functools.lru_cache(None)
def density_cases():
    """sigma sums, mass, rho0, inv_sigma0: random; sums that land on the 1e-12 floor from both sides; a negative contact sum.
    -> dict(cols [5][n], exact [n], np [n], floored [n] (exactly), near_floor [n])."""
    rng = np.random.default_rng(108)
    n = N_RANDOM
    rho0, isig0 = 1.0, 0.0025
    s_in, s_ct = rng.uniform(300.0, 500.0, n), rng.uniform(0.0, 60.0, n) * 0.0025
    mass = np.full(n, 0.0025)
    # rho = s_in rho0 isig0 + s_ct rho0^2 isig0 / mass; with rho0 = 1, isig0 = 2^-9, mass = 2^-9 every operation is exact:
    # rho = s_in 2^-9 + s_ct
    e_isig, e_mass, t = 2.0 ** -9, 2.0 ** -9, 1e-12
    edge = [(0.0, t), (0.0, na(t, 1.0)), (0.0, na(t, 0.0)), (t * 512.0, 0.0), (400.0, -0.5), (400.0, -400.0 * e_isig), (0.0, 0.0),
            (1.0, -1.0)]
    cols = [np.concatenate([s_in, [v[0] for v in edge]]), np.concatenate([s_ct, [v[1] for v in edge]]),
            np.concatenate([mass, np.full(len(edge), e_mass)]), np.full(n + len(edge), rho0),
            np.concatenate([np.full(n, isig0), np.full(len(edge), e_isig)])]
    exact, floored = [], []
    for a, b, m, r0, s0 in zip(*cols):
        a, b, m, r0, s0 = F(a), F(b), F(m), F(r0), F(s0)
        rho = a * r0 * s0 + b * r0 * r0 * s0 / m
        floored.append(rho <= F(1e-12))
        exact.append(r0 if rho <= F(1e-12) else rho)
    a, b, m, r0, s0 = cols
    rho = a * r0 * s0
    rho = rho + b * r0 * r0 * s0 / m
    rho = np.where(rho <= 1e-12, r0, rho)
    return dict(cols=cols, exact=exact, floored=np.array(floored), np=rho, n_random=n)


@functools.lru_cache(None)
def half_state_cases():
    """rho, drho, dt, rho0, p0: random, and rho + dt / 2 drho on both sides of 1e-10 (and on it).
    -> dict(cols [5][n], exact [n][2], np [n][2], floored [n])."""
    rng = np.random.default_rng(109)
    n = N_RANDOM
    rho, drho, dt = rng.uniform(0.9, 1.1, n), rng.uniform(-40.0, 40.0, n), rng.uniform(1e-5, 2e-3, n)
    t = 1e-10
    # dt = 2, drho = -1: rho_half = rho - 1 exactly (Sterbenz) for rho in [0.5, 2]
    edge = [(1.0 + t, -1.0, 2.0), (na(1.0, 2.0), -1.0, 2.0), (1.0, -1.0, 2.0), (t, 0.0, 1e-3), (na(t, 0.0), 0.0, 1e-3), (na(t, 1.0), 0.0, 1e-3),
            (1.0, -3.0, 1.0)]
    cols = [np.concatenate([rho, [v[0] for v in edge]]), np.concatenate([drho, [v[1] for v in edge]]),
            np.concatenate([dt, [v[2] for v in edge]]), np.full(n + len(edge), 1.0), np.full(n + len(edge), 225.0)]
    cols[3][:n:2] = 1000.0  # (both densities the suite runs with)
    cols[0][:n:2] *= 1000.0
    exact, floored = [], []
    for r, d, s, r0, p0 in zip(*cols):
        r, d, s, r0, p0 = F(r), F(d), F(s), F(r0), F(p0)
        rh = r + Fraction(1, 2) * s * d
        floored.append(rh < F(1e-10))
        if rh < F(1e-10):
            rh = r0
        exact.append([rh, p0 * (rh / r0 - 1)])
    r, d, s, r0, p0 = cols
    rh = r + 0.5 * s * d
    rh = np.where(rh < 1e-10, r0, rh)
    return dict(cols=cols, exact=exact, floored=np.array(floored), np=np.stack([rh, p0 * (rh / r0 - 1.0)], 1))


@functools.lru_cache(None)
def eos_cases():
    rng = np.random.default_rng(110)
    n = N_RANDOM
    rho0 = np.where(np.arange(n + 3) % 2 == 0, 1.0, 1000.0)
    rho = rho0 * np.concatenate([rng.uniform(0.8, 1.3, n), [1.0, 1.0, na(1.0, 2.0)]])  # rho = rho0: exactly zero
    p0 = np.full(n + 3, 225.0) * rho0
    exact = [F(c) * (F(a) / F(b) - 1) for a, b, c in zip(rho, rho0, p0)]
    return dict(cols=[rho, rho0, p0], exact=exact, np=p0 * (rho / rho0 - 1.0))


def rel_bound_rule(np_err_worst):
    """The rule of the spline forms, for the other rational formulas: twice numpy-double's own worst error plus 2 eps of scale."""
    return 2.0 * np_err_worst + 2.0


# ------------------------------------------------------------------------------------------------------------------
# B. geometry and the clock
# ------------------------------------------------------------------------------------------------------------------
DL_CASES = (3.0, 1.5, 0.7)


@functools.lru_cache(None)
def wrap_cases(DL):
    """x for wrap_x: the listed edges plus random over a few periods -> dict(x, exact (Fractions), np, returns_DL: mask of the
    inputs whose result is DL itself -- tiny negative x, where x + DL rounds to DL)."""
    rng = np.random.default_rng(201)
    edge = [-DL, -1e-17, -0.0, 0.0, na(DL, 0.0), DL, na(DL, 2 * DL), 2.5 * DL, -0.25 * DL, -1e-300, -ulp(DL) / 4, 2 * DL, -2 * DL]
    x = np.concatenate([edge, rng.uniform(-3.0 * DL, 4.0 * DL, N_RANDOM)])
    exact = [F(v) - math.floor(F(v) / F(DL)) * F(DL) for v in x]
    w = x - np.floor(x / DL) * DL
    return dict(x=x, exact=exact, np=w, returns_DL=w == DL)


# (name, ncx, ncy, x0, y0, DL, cs): columns tile DL exactly (inv_csx = ncx / DL), rows are cs high (inv_csy = 1 / cs), as the
# context builds its grid.  The periodic grid of dp = 0.05 / DL = 3 at a skin of 1.05 h (cs = 3.05 h: 15 columns, 8 rows from the
# lowest wall particle), and a 7 x 5 window that starts left of zero, as a slab's does
GRIDS = (("dp0.05_DL3", 15, 8, 0.0, -0.125, 3.0, 3.05 * 1.3 * 0.05), ("7x5", 7, 5, -0.3, -0.1, 2.1, 0.25))


@functools.lru_cache(None)
def cell_cases(which):
    """x, y for cell_of on GRIDS[which]: every cell edge and one ulp either side, the ends of the grid, random points inside and
    a little outside (clamped).  -> dict(grid, dpar, ipar, x, y, cx, cy exact, edge_dist_x / _y: distance to the nearest cell
    edge), x and y sorted so that monotony can be read off the result."""
    name, ncx, ncy, x0, y0, DL, cs = GRIDS[which]
    inv_csx, inv_csy, DH = ncx / DL, 1.0 / cs, ncy * cs  # (DH: the height of the grid)
    rng = np.random.default_rng(202 + which)

    def axis(o, inv, nc, length):
        e = np.array([o + k / inv for k in range(nc + 1)] + [o + k * (length / nc) for k in range(nc + 1)])
        v = np.concatenate([e, na(e, -np.inf), na(e, np.inf), [o - 0.1 * length, o + 1.1 * length]])
        return np.sort(np.concatenate([v, rng.uniform(o - 0.1 * length, o + 1.1 * length, 800 - v.size)]))

    x, y = axis(x0, inv_csx, ncx, DL), axis(y0, inv_csy, ncy, DH)

    def exact(v, o, inv, nc):
        c, dist = [], []
        for t in v:
            s = (F(t) - F(o)) * F(inv)
            c.append(min(max(math.floor(s), 0), nc - 1))
            dist.append(float(abs(s - round(s)) / F(inv)))
        return np.array(c), np.array(dist)

    cx, ddx = exact(x, x0, inv_csx, ncx)
    cy, ddy = exact(y, y0, inv_csy, ncy)
    return dict(name=name, ncx=ncx, ncy=ncy, DL=DL, DH=DH, dpar=(x0, y0, inv_csx, inv_csy, DL), x=x, y=y, cx=cx, cy=cy, edge_dist_x=ddx,
                edge_dist_y=ddy)


def min_image_numpy(dx, DL, half):
    return np.where(dx > half, dx - DL, np.where(dx < -half, dx + DL, dx))


@functools.lru_cache(None)
def min_image_inputs(DL):
    rng = np.random.default_rng(203)
    half = 0.5 * DL
    edge = [half, -half, na(half, DL), na(-half, -DL), na(half, 0.0), na(-half, 0.0), 0.0, -0.0, DL, -DL, na(DL, 0.0)]
    return np.concatenate([edge, rng.uniform(-DL, DL, N_RANDOM)])


@functools.lru_cache(None)
def column_cases():
    """Every (ncx, cx, ox, periodic) with ncx in {1, 2, 3, 4, 7} -> int columns [4][n]."""
    rows = [(ncx, cx, ox, per) for ncx in (1, 2, 3, 4, 7) for cx in range(ncx) for ox in (-1, 0, 1) for per in (0, 1)]
    return np.array(rows, dtype=np.int32).T


def expected_columns(ncx, cx, periodic):
    """The distinct columns among cx - 1, cx, cx + 1 (modulo ncx on a periodic grid, inside the window on an open one)."""
    cols = [cx - 1, cx, cx + 1]
    return sorted({c % ncx for c in cols} if periodic else {c for c in cols if 0 <= c < ncx})


@functools.lru_cache(None)
def rebin_cases():
    """Every (ncx, ncy, periodic, c_old, c_new) on grids up to 5 x 4 -> (int columns [5][n], expected [n])."""
    rows, exp = [], []
    for ncx in range(1, 6):
        for ncy in range(1, 5):
            for per in (0, 1):
                for c_old in range(ncx * ncy):
                    for c_new in range(ncx * ncy):
                        ox, oy, nx, ny = c_old // ncy, c_old % ncy, c_new // ncy, c_new % ncy
                        dx = abs(nx - ox)
                        if per and dx == ncx - 1:
                            dx = 1
                        rows.append((ncx, ncy, per, c_old, c_new))
                        exp.append(int(dx <= 1 and abs(ny - oy) <= 1))
    return np.array(rows, dtype=np.int32).T, np.array(exp)


def next_dt_numpy(t, t_target, t_end, vmax, h, c_f, dt_viscous, dt_body, n_in):
    remain = np.fmin(t_target - t, t_end - t)
    dt_ac = 0.25 * h / np.fmax(c_f + vmax, 1e-12)
    single = np.fmax(np.fmin(np.fmin(dt_ac, dt_viscous), np.fmin(dt_body, remain)), 1e-12)
    dt_adv = 0.25 * h / np.fmax(vmax, 1e-12)
    Dt = np.fmin(np.fmin(np.fmin(dt_adv, dt_viscous), np.fmin(dt_body, remain)), n_in * dt_ac)
    return np.where(n_in > 1, np.fmax(Dt / n_in, 1e-12), single)


# one input per binding limit: name -> (t, t_target, t_end, vmax, h, c_f, dt_viscous, dt_body); with n_in = 1 and 3
NEXT_DT_CASES = dict(
    acoustic=(0.1, 5.0, 9.0, 1.5, 0.065, 15.0, 0.5, 0.4),
    viscous=(0.1, 5.0, 9.0, 1.5, 0.065, 15.0, 2e-4, 0.4),
    body=(0.1, 5.0, 9.0, 1.5, 0.065, 15.0, 0.5, 3e-4),
    remain_target=(4.99995, 5.0, 9.0, 1.5, 0.065, 15.0, 0.5, 0.4),
    remain_end=(8.99995, 15.0, 9.0, 1.5, 0.065, 15.0, 0.5, 0.4),
    floor_remain_zero=(5.0, 5.0, 9.0, 1.5, 0.065, 15.0, 0.5, 0.4),
    floor_remain_negative=(5.5, 5.0, 9.0, 1.5, 0.065, 15.0, 0.5, 0.4),
    advective_n3=(0.1, 5.0, 9.0, 40.0, 0.065, 15.0, 0.5, 0.4),  # n_in = 3: the advection scale binds before 3 acoustic steps
    at_rest=(0.0, 5.0, 9.0, 0.0, 0.065, 15.0, 0.5, 0.4),
)


# ------------------------------------------------------------------------------------------------------------------
# C. list codecs and the tile layout
# ------------------------------------------------------------------------------------------------------------------
K_DELTA_MAX, K_CODED_DELTA_MAX, K_CODE_BIAS, K_SLOT_CODES, K_FORCE_SLOTS = 32767, 32500, 33000, 480, 464


def wrap_index(k, n):
    return k + n if k < 0 else (k - n if k >= n else k)


@functools.lru_cache(None)
def row_count_cases(lpp, capacity):
    """Every cnt 0 .. capacity, cnt_fl in {0, 1, cnt // 2, cnt - 1, cnt}, every sub -> (int columns [3][n], rows, fluid rows)."""
    rows = []
    for cnt in range(capacity + 1):
        for fl in sorted({0, 1, cnt // 2, cnt - 1, cnt}):
            if 0 <= fl <= cnt:
                rows += [(cnt, fl, sub) for sub in range(lpp)]
    a = np.array(rows, dtype=np.int32).T
    return a, np.array([len(range(s, c, lpp)) for c, f, s in rows]), np.array([len(range(s, f, lpp)) for c, f, s in rows])


@functools.lru_cache(None)
def encode_cases():
    """(k, i, n, periodic, limit) over n in {2, 3, 101, 65 535, 65 536, 70 001}: all pairs of the small n; of the large, i at the
    ends and in the middle against every k that puts the stored difference on, one inside and one beyond each limit and the
    half period.  -> int columns [5][n]"""
    rows = []
    for n in (2, 3, 101):
        rows += [(k, i, n, per, lim) for k in range(n) for i in range(n) for per in (0, 1) for lim in (K_DELTA_MAX, K_CODED_DELTA_MAX)]
    for n in (65535, 65536, 70001):
        for i in (0, 1, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1):
            for lim in (K_DELTA_MAX, K_CODED_DELTA_MAX):
                ds = {s * (lim + o) for s in (-1, 1) for o in (-1, 0, 1, 2)} | {s * (n // 2 + o) for s in (-1, 1) for o in (-1, 0, 1)} | {0, 1, -1}
                for d in sorted(ds):
                    for per in (0, 1):
                        k = (i + d) % n if per else i + d
                        if 0 <= k < n:
                            rows.append((k, i, n, per, lim))
    return np.array(sorted(set(rows)), dtype=np.int32).T


def tile_index(m, sl):
    lo0, lo1, lo2, n0, n1, n2 = m
    return lo0 + sl if sl < n0 else (lo1 + sl - n0 if sl < n0 + n1 else lo2 + sl - n0 - n1)


def tile_capped(m, cap):
    lo0, lo1, lo2, n0, n1, n2 = m
    c0 = min(n0, cap); c1 = min(n1, cap - c0); c2 = min(n2, cap - c0 - c1)
    return (lo0, lo1, lo2, c0, c1, c2)


@functools.lru_cache(None)
def tile_layouts():
    """(lo0, lo1, lo2, len0, len1, len2) of three disjoint index ranges, in any order in memory: 200 random layouts, an empty first /
    second / third range, totals of exactly kSlotCodes, kForceSlots and one more, adjacent ranges."""
    rng = np.random.default_rng(301)
    out = []
    for _ in range(200):
        lens = rng.integers(0, 230, 3)
        gaps = rng.integers(0, 50, 3) * rng.integers(0, 2, 3)  # (a zero gap: adjacent ranges)
        order = rng.permutation(3)
        lo, pos = [0, 0, 0], int(rng.integers(0, 100000))
        for j in order:
            pos += int(gaps[j]); lo[j] = pos; pos += int(lens[j])
        out.append((lo[0], lo[1], lo[2], int(lens[0]), int(lens[1]), int(lens[2])))
    out += [(500, 500, 900, 0, 120, 130), (500, 900, 900, 150, 0, 130), (500, 100, 0, 150, 120, 0), (0, 0, 0, 0, 0, 0),
            (1000, 700, 1300, 200, 150, 130), (1000, 700, 1300, 200, 150, 114), (1000, 700, 1300, 200, 150, 131), (1000, 700, 1300, 200, 150, 115),
            (100, 0, 300, 200, 100, 50), (0, 100, 300, 100, 200, 50), (40000, 39000, 41000, 480, 200, 200), (7, 0, 12, 5, 7, 3)]
    return tuple(out)


# ranges that overlap (no layout of tile_ranges does): the first range that holds k names its slot -- the smallest one, the one a
# capped prefix of the layout still stages.  The first: an empty first range with lo0 == lo1.
TILE_OVERLAPS = ((500, 500, 560, 0, 100, 100), (500, 450, 520, 100, 100, 100), (0, 0, 0, 50, 60, 70))


def tile_slot_smallest(m, k):
    for sl in range(m[3] + m[4] + m[5]):
        if tile_index(m, sl) == k:
            return sl
    return -1


@functools.lru_cache(None)
def tile_ranges_cases():
    """Synthetic sorted layouts for tile_ranges: (name, ncx, ncy, periodic, cell [n], start [ncells + 1]) with uneven columns, an
    empty column, ncx in {1, 2, 3, 5}."""
    rng = np.random.default_rng(302)
    out = []
    for ncx, ncy, per, mean, empty_col in ((1, 6, 1, 40, None), (2, 5, 1, 60, None), (3, 7, 1, 30, None), (5, 4, 1, 70, 2), (5, 6, 0, 25, 3),
                                          (3, 5, 0, 45, None)):
        cnt = rng.integers(0, 2 * mean, ncx * ncy)
        if empty_col is not None:
            cnt[empty_col * ncy:(empty_col + 1) * ncy] = 0
        start = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        cell = np.repeat(np.arange(ncx * ncy), cnt).astype(np.int32)
        out.append(("%dx%d%s" % (ncx, ncy, "p" if per else "o"), ncx, ncy, per, cell, start))
    return tuple(out)


def tile_ranges_rule(lpp, ncx, ncy, periodic, cell, start, blk, n_now, cap):
    """The layout of workgroup blk: the rows of its own column its particles span, widened by one row either way, in the own
    column, the left one and the right one (where there is a distinct one), each cut to what is left of cap."""
    per = 256 // lpp
    p0 = blk * per
    if p0 >= n_now:
        return (0, 0, 0, 0, 0, 0)
    p1 = min(p0 + per, n_now) - 1
    cx, r_lo = divmod(int(cell[p0]), ncy)
    r_hi = int(cell[p1]) % ncy if int(cell[p1]) // ncy == cx else ncy - 1
    ra, rb = max(r_lo - 1, 0), min(r_hi + 1, ncy - 1) + 1
    rng = {}
    for ox in (-1, 0, 1):
        col = cx + ox
        ok = True
        if periodic:
            if (ncx == 1 and ox != 0) or (ncx == 2 and ox == 1):
                ok = False
            col %= ncx
        elif not 0 <= col < ncx:
            ok = False
        rng[ox] = (int(start[col * ncy + ra]), int(start[col * ncy + rb]) - int(start[col * ncy + ra])) if ok else (0, 0)
    n0 = min(rng[0][1], cap); n1 = min(rng[-1][1], cap - n0); n2 = min(rng[1][1], cap - n0 - n1)
    return (rng[0][0], rng[-1][0], rng[1][0], n0, n1, n2)


# ------------------------------------------------------------------------------------------------------------------
# D. scans
# ------------------------------------------------------------------------------------------------------------------
SCAN_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2048, 8191, 8192)
BIG_SCAN_SIZES = (8193, 16 * 1024 - 1, 16 * 1024, 16 * 1024 + 1, 70000)


def scan_inputs(n, kind, seed=401):
    rng = np.random.default_rng(seed + n)
    if kind == "random":
        return rng.integers(0, 301, n).astype(np.int32)
    c = np.zeros(n, dtype=np.int32)
    if kind == "one_cell":
        c[int(rng.integers(0, n))] = 1234567
    return c


def scan_expected(count):
    return np.concatenate([[0], np.cumsum(count.astype(np.int64))]).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------
# E. bins and fixed point
# ------------------------------------------------------------------------------------------------------------------
def stats_bin_inputs(n_bins, DH):
    """y in [0, DH]: every edge k * bin_w and one ulp either side, 0, DH, random."""
    rng = np.random.default_rng(501 + n_bins)
    bin_w = DH / n_bins
    e = np.arange(n_bins + 1) * bin_w
    y = np.concatenate([e, na(e, -np.inf), na(e, np.inf), [0.0, DH], rng.uniform(0.0, DH, 2000)])
    return bin_w, y[(y >= 0.0) & (y <= DH)]


def profile_bin(y, DH, n_bins):
    """profile.compute_binned_profile_mean's bin of y in [0, DH]."""
    edges = np.linspace(0.0, DH, n_bins + 1)
    return np.minimum(np.searchsorted(edges, y, side="right") - 1, n_bins - 1)


def band_inputs(DL, xc, hw):
    rng = np.random.default_rng(502)
    k = np.arange(-2, 4) * DL
    on_edge = [xc + hw, xc - hw, xc + hw + DL, xc - hw - DL, na(xc + hw, np.inf), na(xc - hw, -np.inf), xc, xc + DL]
    return np.concatenate([k, na(k, -np.inf), na(k, np.inf), on_edge, -rng.uniform(0.0, 2 * DL, 500), rng.uniform(-DL, 3 * DL, 3000)])


def pair_bin_inputs(n_bins, r_max):
    """r2 < r_max^2: exactly on every squared edge, one ulp either side, random."""
    rng = np.random.default_rng(503 + n_bins)
    bin_w = r_max / n_bins
    e = np.arange(n_bins, dtype=np.float64) * bin_w
    e2 = np.append(e * e, r_max * r_max)
    r2 = np.concatenate([e2, na(e2, -np.inf), na(e2, np.inf), rng.uniform(0.0, r_max, 3000) ** 2, [0.0]])
    return bin_w, e2, r2[(r2 >= 0.0) & (r2 < e2[-1])]


def stats_scales(vmax, n):
    """stats_scales of sphx_flow_stats.hpp in Python (as profile.grad_scales states grad_scales): n <= 2^L, 2^e > max(2 vmax,
    2^-60) -> (s1, s2, bound)."""
    L = 0
    while L < 31 and (1 << L) < n:
        L += 1
    x = 2.0 * float(vmax)
    e = int(np.frexp(x if x > 2.0 ** -60 else 2.0 ** -60)[1])
    return 62 - L - e, 62 - L - 2 * e, float(np.ldexp(1.0, e))


SCALE_N = (1, 2, 3, 2 ** 10, 2 ** 10 + 1, 2 ** 20, 2 ** 20 + 1, 2 ** 30, 2 ** 30 + 1, 2 ** 31 - 1)


def scale_vmax(h=None):
    """vmax: 0, subnormal, 2^k and the next double, 1e300, and -- last -- inf and NaN.  With h: also the vmax at which 16 vmax / h is
    a power of two exactly (vmax = h 2^(k-4)), where only the strictness of the bound tells 16 from 15."""
    v = [0.0, 5e-324, 1e-310, 2.0 ** -70, 2.0 ** -61, na(2.0 ** -61, 1.0), 2.0 ** -20, 1.0, na(1.0, 2.0), 1.5, 2.0, na(2.0, 3.0), 8.0, 2.0 ** 40, 1e300]
    if h is not None:
        v += [h * 2.0 ** (k - 4) for k in (-3, 0, 1, 5, 12)]
    return np.array(v + [np.inf, np.nan])
