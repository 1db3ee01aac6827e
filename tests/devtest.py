"""numpy-in / numpy-out bindings of the test-only harness library csrc/libsphx_devtest.so (csrc/sphx_devtest.hip): the small
__device__ functions of the production headers, each called alone on arrays of inputs.

SPHX_DEVTEST_LIB=<path> loads another build of the harness (a deliberately altered header: profiles/r33_device_formulas.txt).
Not a conftest: tests import it."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "sph-poiseuille-flow_amd"
LIB_PATH = os.environ.get("SPHX_DEVTEST_LIB") or os.path.join(ROOT, PKG, "csrc", "libsphx_devtest.so")

# the operations of the element-wise entries, in the order of csrc/sphx_devtest.hip's enum Op
OPS = ("F_RCP_NR F_RSQRT_NR F_PAIR_GEOM F_SPLINE F_SPLINE_DW F_SPLINE_W F_SPLINE_DW_SEL F_SPLINE_DW_IN F_SPLINE_W_SEL "
       "F_KGC_MOMENT_ADD F_CONTINUITY_ADD F_WALL_PAIR F_WALL_PRESSURE_ADD F_KGC_FROM_A F_RIEMANN_BETA F_TRANSPORT_SHIFT "
       "F_DENSITY_FROM_SIGMA F_HALF_STATE F_EOS_PRESSURE "
       "G_WRAP_X G_CELL_OF G_MIN_IMAGE G_NEIGHBOUR_COLUMN G_REBIN_NEAR G_OWNS G_TRACKED_DRIFT2 G_NEXT_DT G_LOOP_CONTINUES "
       "C_LIST_ROW_COUNTS C_ENCODE_DELTA C_WORD_HALVES C_WRAP_INDEX C_TILE_SLOT C_TILE_INDEX C_TILE_CAPPED C_CODED_INDEX "
       "L_GROUP_SUM L_GROUP_EXTREME L_WAVE_MAX L_PAIR_PARTNER L_BLOCK_SCAN_T "
       "B_STATS_BIN B_STATS_IN_BAND B_PAIR_R2 B_PAIR_EDGE2 B_PAIR_BIN B_STATS_SCALES B_GRAD_SCALES B_QUANTISE").split()
OP = {name: k for k, name in enumerate(OPS)}
FAMILY = {"F": "sphx_devtest_formulas", "G": "sphx_devtest_geometry", "C": "sphx_devtest_codecs", "L": "sphx_devtest_lanes",
          "B": "sphx_devtest_bins"}
ENTRIES = tuple(FAMILY.values()) + ("sphx_devtest_op_info", "sphx_devtest_device_count", "sphx_devtest_put_delta",
                                    "sphx_devtest_tile_ranges", "sphx_devtest_scan_counts", "sphx_devtest_big_scan")
BLOCK = 256  # the lane and block operations (L_*) take whole blocks

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s has not been built (__graft_entry__.build())" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name in FAMILY.values():
            f = getattr(L, name)
            f.restype = C.c_int
            f.argtypes = [C.c_int, _dp, C.c_int, _ip, C.c_int, _dp, C.c_int, _ip, C.c_int, C.c_int, _dp, C.c_int, _ip, C.c_int]
        L.sphx_devtest_op_info.restype = C.c_int
        L.sphx_devtest_op_info.argtypes = [C.c_int, _ip]
        L.sphx_devtest_device_count.restype = C.c_int
        L.sphx_devtest_device_count.argtypes = []
        L.sphx_devtest_put_delta.restype = C.c_int
        L.sphx_devtest_put_delta.argtypes = [_ip, C.c_int, C.c_int, _ip, _ip, _ip, _ip, _ip, C.c_int]
        L.sphx_devtest_tile_ranges.restype = C.c_int
        L.sphx_devtest_tile_ranges.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, C.c_int, C.c_int, C.c_int, _ip]
        for name in ("sphx_devtest_scan_counts", "sphx_devtest_big_scan"):
            f = getattr(L, name)
            f.restype = C.c_int
            f.argtypes = [_ip, _ip, C.c_int]
        _LIB = L
    return _LIB


def op_info(op):
    """(columns: double in, int in, double out, int out), number of operations -- the library's own table."""
    info = (C.c_int * 4)()
    n_ops = lib().sphx_devtest_op_info(op, info)
    return tuple(info), n_ops


def device_count():
    return lib().sphx_devtest_device_count()


class DevtestError(RuntimeError):
    pass


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _cols(cols, conv, n):
    if not cols:
        return conv(np.zeros(0)), 0
    return conv(np.stack([np.broadcast_to(conv(c), (n,)) for c in cols])), len(cols)


def call(name, d=(), i=(), dpar=(), ipar=(), n=None, check=True):
    """Operation `name` on n elements: d / i are the double / int input columns (arrays of length n, or scalars) -> (list of double
    output columns, list of int output columns).  check=False: -> the HIP error code instead of raising."""
    if n is None:
        n = max(np.size(c) for c in list(d) + list(i))
    op = OP[name]
    (kdi, kii, kdo, kio), _ = op_info(op)
    din, ndi = _cols(d, _d, n)
    iin, nii = _cols(i, _i, n)
    dout, iout = np.zeros((kdo, n)), np.zeros((kio, n), dtype=np.int32)
    dp, ip = _d(dpar), _i(ipar)
    err = getattr(lib(), FAMILY[name[0]])(op, din.ctypes.data_as(_dp), ndi, iin.ctypes.data_as(_ip), nii, dout.ctypes.data_as(_dp), kdo,
                                         iout.ctypes.data_as(_ip), kio, n, dp.ctypes.data_as(_dp), dp.size, ip.ctypes.data_as(_ip),
                                         ip.size)
    if not check:
        return err
    if err != 0:
        raise DevtestError("%s: HIP error %d" % (name, err))
    return list(dout), list(iout)


def call_whole_blocks(name, d=(), i=(), dpar=(), ipar=()):
    """An L_* operation on arrays padded with zeros to whole blocks; the padding is cut off the results."""
    n = max(np.size(c) for c in list(d) + list(i))
    m = -(-n // BLOCK) * BLOCK
    pad = lambda c, conv: np.concatenate([conv(c), conv(np.zeros(m - n))])
    do, io = call(name, [pad(c, _d) for c in d], [pad(c, _i) for c in i], dpar, ipar, n=m)
    return [c[:n] for c in do], [c[:n] for c in io]


def put_delta(pk, rows, stride, row, col, d, check=True):
    """pk: the words before -> (the words after, delta_of_row, code_of_row of every element)."""
    pk, row, col, d = _i(pk).copy(), _i(row), _i(col), _i(d)
    n = row.size
    delta, code = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    err = lib().sphx_devtest_put_delta(pk.ctypes.data_as(_ip), rows, stride, row.ctypes.data_as(_ip), col.ctypes.data_as(_ip),
                                       d.ctypes.data_as(_ip), delta.ctypes.data_as(_ip), code.ctypes.data_as(_ip), n)
    if not check:
        return err
    if err != 0:
        raise DevtestError("put_delta: HIP error %d" % err)
    return pk, delta, code


def tile_ranges(lpp, ncx, ncy, periodic, cell, start, n_now, cap, n_blk, check=True):
    """-> [n_blk][6] = lo0 lo1 lo2 len0 len1 len2 of tile_ranges<lpp>(blk = 0 .. n_blk-1)."""
    cell, start = _i(cell), _i(start)
    if cell.size < n_now or start.size != ncx * ncy + 1:
        raise ValueError("cell[n_now], start[ncells + 1]")
    out = np.zeros((n_blk, 6), dtype=np.int32)
    err = lib().sphx_devtest_tile_ranges(lpp, ncx, ncy, int(periodic), cell.ctypes.data_as(_ip), start.ctypes.data_as(_ip), n_now, cap,
                                         n_blk, out.ctypes.data_as(_ip))
    if not check:
        return err
    if err != 0:
        raise DevtestError("tile_ranges: HIP error %d" % err)
    return out


def _scan(entry, count):
    count = _i(count)
    start = np.zeros(count.size + 1, dtype=np.int32)
    err = getattr(lib(), entry)(count.ctypes.data_as(_ip), start.ctypes.data_as(_ip), count.size)
    if err != 0:
        raise DevtestError("%s: HIP error %d" % (entry, err))
    return start


def scan_counts(count):
    return _scan("sphx_devtest_scan_counts", count)


def big_scan(count):
    return _scan("sphx_devtest_big_scan", count)

