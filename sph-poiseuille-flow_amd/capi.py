"""ctypes binding of libsphx.so (include/sphx.h).  Plumbing only: numpy float64 column-major arrays
in, numpy arrays out.  There is no CPU fallback: if the shared library is missing or no HIP device is
present the calls raise."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .profile import (DENS_FIELDS, DENS_MAX_HIST, DENS_MAX_WORDS, FIELD_MAP_PLANES, GRAD_FIELDS, GRAD_MAX_BINS,
                      STATS_FIELDS, dens_stats_profiles, field_map_means, flow_stats_profile, grad_stats_profiles,
                      pair_dist_profiles, pair_edges, profile_series_profiles)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPHX_LIB") or os.path.join(HERE, "csrc", "libsphx.so")  # SPHX_LIB: experiment builds
_dp = C.POINTER(C.c_double)

SPHX_OK = 0
SPHX_ERR_ARG, SPHX_ERR_DEVICE, SPHX_ERR_STATE, SPHX_ERR_DIVERGED, SPHX_ERR_GRID = -1, -2, -3, -4, -5


class SphxError(RuntimeError):
    """Raised for any non-zero status; .identifier is the MEX-style error id."""

    def __init__(self, code, identifier, message):
        super().__init__(f"[{identifier}] {message} (status {code})")
        self.code = code
        self.identifier = identifier
        self.message = message


class SphxParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("DL", "DH", "dp", "h", "rho0", "mu", "c_f", "p0", "inv_sigma0",
                                           "gravity_g", "transport_coeff", "t_end")] + \
               [("sort_interval", C.c_int32), ("lanes_per_particle", C.c_int32),
                ("steps_per_graph", C.c_int32), ("dual_rate", C.c_int32), ("rebuild_every", C.c_int32),
                ("dynamic_rebin", C.c_int32), ("skin_h", C.c_double)]


class SphxFlowStatsConfig(C.Structure):
    _fields_ = [("n_bins", C.c_int32), ("every", C.c_int32), ("t_from", C.c_double), ("n_bands", C.c_int32),
                ("band_x", C.c_double * 2), ("band_hw", C.c_double * 2)]


class SphxHistoryConfig(C.Structure):
    _fields_ = [("every", C.c_int32), ("capacity", C.c_int32), ("t_from", C.c_double)]


class SphxFieldMapConfig(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("every", C.c_int32), ("with_walls", C.c_int32), ("t_from", C.c_double)]


# a record of the step history (include/sphx.h section 2d), in the order the library writes it
HISTORY_FIELDS = ("step", "t", "dt", "vmax", "tau_bottom", "tau_top", "kinetic_energy", "u_bulk")


class SphxProbesConfig(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("every", C.c_int32), ("capacity", C.c_int32), ("with_walls", C.c_int32),
                ("t_from", C.c_double), ("points", _dp)]


# the values of a probe (include/sphx.h section 2h), in the order the library writes them
PROBE_FIELDS = ("weight", "u_x", "u_y", "rho")
PROBE_MAX_POINTS = 4096


class SphxProfileSeriesConfig(C.Structure):
    _fields_ = [("n_bins", C.c_int32), ("every", C.c_int32), ("capacity", C.c_int32), ("t_from", C.c_double),
                ("n_bands", C.c_int32), ("band_x", C.c_double * 2), ("band_hw", C.c_double * 2)]


class SphxPairDistConfig(C.Structure):
    _fields_ = [("n_bins", C.c_int32), ("every", C.c_int32), ("t_from", C.c_double), ("r_max", C.c_double),
                ("y_margin", C.c_double), ("with_walls", C.c_int32), ("n_bands", C.c_int32), ("band_x", C.c_double * 2),
                ("band_hw", C.c_double * 2)]


PAIR_DIST_MAX_BINS = 1024


class SphxGradStatsConfig(C.Structure):
    _fields_ = [("n_bins", C.c_int32), ("every", C.c_int32), ("t_from", C.c_double), ("det_min", C.c_double),
                ("with_walls", C.c_int32), ("n_bands", C.c_int32), ("band_x", C.c_double * 2), ("band_hw", C.c_double * 2)]


class SphxTracersConfig(C.Structure):
    _fields_ = [("n_tracers", C.c_int32), ("every", C.c_int32), ("capacity", C.c_int32), ("t_from", C.c_double),
                ("ids", C.POINTER(C.c_int32))]


# the values of a tracer (include/sphx.h section 2p), in the order the library writes them
TRACER_FIELDS = ("x", "y", "u_x", "u_y")


class SphxDensStatsConfig(C.Structure):
    _fields_ = [("n_bins", C.c_int32), ("every", C.c_int32), ("t_from", C.c_double), ("n_hist", C.c_int32), ("n_bands", C.c_int32),
                ("hist_range", C.c_double), ("delta_bound", C.c_double), ("band_x", C.c_double * 2), ("band_hw", C.c_double * 2)]


class SphxModesConfig(C.Structure):
    _fields_ = [("mx", C.c_int32), ("ny", C.c_int32), ("every", C.c_int32), ("capacity", C.c_int32), ("t_from", C.c_double)]


# the fields and bases of a mode (include/sphx.h section 2t), in the order the library writes them
MODE_FIELDS = ("n", "ux", "uy")
MODE_BASES = ("cc", "sc", "cs", "ss")
MODES_MAX = 16


class SphxStatus(C.Structure):
    _fields_ = [("t", C.c_double), ("dt_last", C.c_double), ("dt_next", C.c_double), ("vmax", C.c_double),
                ("step", C.c_int64), ("done", C.c_int32), ("device_status", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


EXPORTS = [
    "sphx_version", "sphx_last_error", "sphx_last_error_id", "sphx_device_count", "sphx_set_device",
    "sphx_pool_stats", "sphx_pool_scrub", "sphx_pool_poison_on_free", "sphx_pool_poison_stats",
    "sphx_neighbor_search", "sphx_neighbor_fetch", "sphx_density_correction", "sphx_viscous_force",
    "sphx_transport_correction", "sphx_integration_1st", "sphx_integration_2nd",
    "sphx_integration_verlet", "sphx_advance_shell_step", "sphx_wall_shear_monitor",
    "sphx_ctx_create", "sphx_ctx_destroy", "sphx_ctx_advance", "sphx_ctx_enqueue_steps", "sphx_ctx_sync",
    "sphx_ctx_prepare_steps", "sphx_ctx_graph_stats",
    "sphx_ctx_download", "sphx_ctx_monitor", "sphx_ctx_neighbor_list", "sphx_ctx_profile_enable",
    "sphx_ctx_profile_read", "sphx_ctx_info", "sphx_ctx_tuning", "sphx_ctx_block_size", "sphx_ctx_substeps", "sphx_ctx_schedule", "sphx_ctx_kernel_forms", "sphx_ctx_grid_policy", "sphx_ctx_time_kernel",
    "sphx_ctx_flow_stats_enable", "sphx_ctx_flow_stats_disable", "sphx_ctx_flow_stats_reset", "sphx_ctx_flow_stats_sample",
    "sphx_ctx_flow_stats_read",
    "sphx_ctx_history_enable", "sphx_ctx_history_disable", "sphx_ctx_history_read",
    "sphx_ctx_field_map_enable", "sphx_ctx_field_map_disable", "sphx_ctx_field_map_reset", "sphx_ctx_field_map_sample",
    "sphx_ctx_field_map_read",
    "sphx_ctx_probes_enable", "sphx_ctx_probes_disable", "sphx_ctx_probes_sample", "sphx_ctx_probes_read",
    "sphx_ctx_profile_series_enable", "sphx_ctx_profile_series_disable", "sphx_ctx_profile_series_sample",
    "sphx_ctx_profile_series_read",
    "sphx_ctx_pair_dist_enable", "sphx_ctx_pair_dist_disable", "sphx_ctx_pair_dist_reset", "sphx_ctx_pair_dist_sample",
    "sphx_ctx_pair_dist_read",
    "sphx_ctx_grad_stats_enable", "sphx_ctx_grad_stats_disable", "sphx_ctx_grad_stats_reset", "sphx_ctx_grad_stats_sample",
    "sphx_ctx_grad_stats_read",
    "sphx_ctx_tracers_enable", "sphx_ctx_tracers_disable", "sphx_ctx_tracers_sample", "sphx_ctx_tracers_read",
    "sphx_ctx_dens_stats_enable", "sphx_ctx_dens_stats_disable", "sphx_ctx_dens_stats_reset", "sphx_ctx_dens_stats_sample",
    "sphx_ctx_dens_stats_read",
    "sphx_ctx_modes_enable", "sphx_ctx_modes_disable", "sphx_ctx_modes_sample", "sphx_ctx_modes_read",
    "sphx_slab_create", "sphx_slab_layout", "sphx_slab_local_vmax", "sphx_slab_prepare", "sphx_slab_compute",
    "sphx_slab_finish", "sphx_slab_sync", "sphx_slab_snapshot", "sphx_comm_available", "sphx_comm_unique_id", "sphx_comm_selftest", "sphx_comm_selftest_graph", "sphx_slab_comm_init",
    "sphx_slab_comm_destroy", "sphx_slab_run", "sphx_slab_group_run", "sphx_slab_graph_prepare",
    "sphx_slab_flow_stats_enable", "sphx_slab_flow_stats_disable", "sphx_slab_flow_stats_reset", "sphx_slab_flow_stats_read",
    "sphx_slab_history_enable", "sphx_slab_history_disable", "sphx_slab_history_read",
    "sphx_slab_field_map_enable", "sphx_slab_field_map_disable", "sphx_slab_field_map_reset", "sphx_slab_field_map_read",
    "sphx_slab_probes_enable", "sphx_slab_probes_disable", "sphx_slab_probes_read",
    "sphx_slab_pseries_enable", "sphx_slab_pseries_disable", "sphx_slab_pseries_read",
    "sphx_slab_pairs_enable", "sphx_slab_pairs_disable", "sphx_slab_pairs_reset", "sphx_slab_pairs_read",
    "sphx_slab_gstats_enable", "sphx_slab_gstats_disable", "sphx_slab_gstats_reset", "sphx_slab_gstats_read",
    "sphx_slab_tracers_enable", "sphx_slab_tracers_disable", "sphx_slab_tracers_read",
    "sphx_slab_dstats_enable", "sphx_slab_dstats_disable", "sphx_slab_dstats_reset", "sphx_slab_dstats_read",
    "sphx_batch_create", "sphx_batch_destroy", "sphx_batch_advance", "sphx_batch_enqueue_steps", "sphx_batch_sync",
    "sphx_batch_download", "sphx_batch_monitor", "sphx_batch_info", "sphx_batch_graph_stats",
    "sphx_batch_flow_stats_enable", "sphx_batch_flow_stats_disable", "sphx_batch_flow_stats_reset",
    "sphx_batch_flow_stats_sample", "sphx_batch_flow_stats_read",
    "sphx_batch_history_enable", "sphx_batch_history_disable", "sphx_batch_history_read",
    "sphx_batch_field_map_enable", "sphx_batch_field_map_disable", "sphx_batch_field_map_reset", "sphx_batch_field_map_sample",
    "sphx_batch_field_map_read",
    "sphx_batch_probes_enable", "sphx_batch_probes_disable", "sphx_batch_probes_sample", "sphx_batch_probes_read",
    "sphx_batch_profile_series_enable", "sphx_batch_profile_series_disable", "sphx_batch_profile_series_sample",
    "sphx_batch_profile_series_read",
    "sphx_batch_pair_dist_enable", "sphx_batch_pair_dist_disable", "sphx_batch_pair_dist_reset", "sphx_batch_pair_dist_sample",
    "sphx_batch_pair_dist_read",
    "sphx_batch_grad_stats_enable", "sphx_batch_grad_stats_disable", "sphx_batch_grad_stats_reset", "sphx_batch_grad_stats_sample",
    "sphx_batch_grad_stats_read",
    "sphx_batch_dens_stats_enable", "sphx_batch_dens_stats_disable", "sphx_batch_dens_stats_reset", "sphx_batch_dens_stats_sample",
    "sphx_batch_dens_stats_read",
    "sphx_batch_tracers_enable", "sphx_batch_tracers_disable", "sphx_batch_tracers_sample", "sphx_batch_tracers_read",
    "sphx_batch_modes_enable", "sphx_batch_modes_disable", "sphx_batch_modes_sample", "sphx_batch_modes_read",
]

_LIB = None


def lib() -> C.CDLL:
    """Load libsphx.so; fail loudly when it has not been built (see __graft_entry__.build)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` "
                              f"(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name in ("sphx_version", "sphx_last_error", "sphx_last_error_id"):
            getattr(L, name).restype = C.c_char_p
        L.sphx_ctx_destroy.restype = None
        L.sphx_batch_destroy.restype = None
        _LIB = L
    return _LIB


def check(rc: int) -> None:
    if rc != SPHX_OK:
        L = lib()
        raise SphxError(rc, (L.sphx_last_error_id() or b"").decode(), (L.sphx_last_error() or b"").decode())


def f64(a, fortran=True):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 2:
        return np.asfortranarray(a) if fortran else np.ascontiguousarray(a)
    return np.ascontiguousarray(a)


def ptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def device_count() -> int:
    return int(lib().sphx_device_count())


def set_device(dev: int) -> None:
    check(lib().sphx_set_device(C.c_int(dev)))


def pool_stats() -> dict:
    """The device-memory pool's counters: cached_bytes, cached_blocks, and the allocations served from the cache (hits) and by
    hipMalloc (misses) since process start.  No device needed: all zeros without one."""
    out = (C.c_uint64 * 4)()
    check(lib().sphx_pool_stats(out))
    return dict(zip(("cached_bytes", "cached_blocks", "hits", "misses"), (int(v) for v in out)))


def pool_scrub(word) -> int:
    """Fill every cached free block of the current device with the 32-bit word; -> the number of blocks filled (0, and no
    device call, with nothing cached).  A diagnostic: results must not depend on what a recycled block held.  Not while a
    stream is capturing."""
    n = C.c_uint64(0)
    check(lib().sphx_pool_scrub(C.c_uint32(int(word)), C.byref(n)))
    return int(n.value)


def pool_poison_on_free(on, word=3) -> None:
    """Test support, off by default: while on, every block that goes back into the pool's cache is first filled with the 32-bit
    word on a stream of the pool's own, which alone is waited for.  Work its former owner left in flight races with the fill,
    so a block released too early shows as wrong numbers (tests/test_gpu_live_neighbours.py).  Not while a stream is capturing."""
    check(lib().sphx_pool_poison_on_free(C.c_int(1 if on else 0), C.c_uint32(int(word))))


def pool_poison_stats() -> dict:
    """Blocks filled by the poison-at-free mode and fills skipped inside a stream capture, since process start.  No device needed."""
    out = (C.c_uint64 * 2)()
    check(lib().sphx_pool_poison_stats(out))
    return dict(filled=int(out[0]), skipped_in_capture=int(out[1]))


def make_params(prm, t_end=None, transport_coeff=None, lanes_per_particle=0, steps_per_graph=0, rebuild_every=0,
                skin_h=0.0, dynamic_rebin=0, dual_rate=0) -> SphxParams:
    return SphxParams(DL=prm.DL, DH=prm.DH, dp=prm.dp, h=prm.h, rho0=prm.rho0, mu=prm.mu, c_f=prm.c_f,
                      p0=prm.p0, inv_sigma0=prm.inv_sigma0, gravity_g=prm.gravity_g,
                      transport_coeff=prm.transport_coeff if transport_coeff is None else transport_coeff,
                      t_end=prm.t_end if t_end is None else t_end, sort_interval=int(prm.sort_interval),
                      lanes_per_particle=int(lanes_per_particle), steps_per_graph=int(steps_per_graph),
                      dual_rate=int(dual_rate), rebuild_every=int(rebuild_every), dynamic_rebin=int(dynamic_rebin), skin_h=float(skin_h))


_FIELDS = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B")


def _field_buffers(nt, fields):
    shapes = dict(pos=(nt, 2), vel=(nt, 2), rho=(nt,), p=(nt,), drho_dt=(nt,), force=(nt, 2),
                  force_prior=(nt, 2), Vol=(nt,), B=(nt, 4))
    out = {k: np.zeros(shapes[k], order="F") for k in fields}
    return out, [ptr(out[k]) if k in out else None for k in _FIELDS]


def _per_member(v, m, name):
    """A scalar for every member, or one value per member."""
    if v is None or np.isscalar(v):
        return [v] * m
    v = list(v)
    if len(v) != m:
        raise SphxError(SPHX_ERR_ARG, "SPHX:Batch:members", f"{name}: one value per member expected ({len(v)} for {m})")
    return v


_STATE = ("pos", "vel", "drho_dt", "mass", "wall_vel")


class _Sampled:
    """What a context, a batch and a slab of a ring bind alike: the flow statistics' sums, the step history's records, the
    profile series' raw records and the pair, gradient and density statistics' sums.  A subclass names its symbol stem, the words
    its profile-series, pair-, gradient- and density-statistics calls carry behind the stem (a slab's are sphx_slab_pseries_*,
    sphx_slab_pairs_*, sphx_slab_gstats_* and sphx_slab_dstats_*), the word of its "not enabled on this ..." errors and whether it
    has many channels: a context or a slab returns one dict / (records, n_dropped) pair, a batch a list with one entry per member."""
    _stem = _where = None
    _series = "profile_series_"
    _pairs = "pair_dist_"
    _grads = "grad_stats_"
    _dens = "dens_stats_"
    _many = False

    def _call(self, name, *args):
        check(getattr(lib(), self._stem + name)(self._h, *args))

    def _channels(self) -> int:
        return self.n_members if self._many else 1

    def _params0(self) -> SphxParams:
        return self.params[0] if self._many else self.params

    def _each(self, per_channel):
        return per_channel if self._many else per_channel[0]

    # ---- flow statistics (include/sphx.h sections 2a, 2c): time-averaged velocity profiles accumulated on the device ----
    def flow_stats_enable(self, n_bins=0, every=1, t_from=0.0, bands=()):
        """Sample the state every `every`-th completed step ending at t >= t_from into n_bins y-bins (0: the reference's
        max(20, round(DH/dp))) of the whole channel (band 0) and of up to two x-bands [(x_centre, half_width), ...]
        (band 1, 2).  (Re)configures and zeroes the sums.  A batch: one config for all members, each sampled on its own clock."""
        cfg = flow_stats_config(n_bins, every, t_from, bands)
        p0 = self._params0()
        n = int(cfg.n_bins) or max(20, int(np.floor(p0.DH / p0.dp + 0.5)))
        self._call("flow_stats_enable", C.byref(cfg))
        self._flow_stats = (n, int(cfg.n_bands) + 1)  # (n_bins, n_bands incl. band 0) while the flow statistics are on

    def flow_stats_disable(self):
        self._call("flow_stats_disable")
        self._flow_stats = None

    def _stats_on(self):
        return _enabled(self._flow_stats, "Stats", f"flow statistics are not enabled on this {self._where}")

    def flow_stats_reset(self):
        self._stats_on()
        self._call("flow_stats_reset")

    def flow_stats_sums(self, band=0):
        """The raw sums of one band: count, sum_ux, sum_ux2, sum_uy, sum_uy2 [n_bins], n_samples, t_first, t_last; a batch: one
        such dict per member, from one read of all members."""
        n_bins, n_bands = self._stats_on()
        if not _is_int(band) or not 0 <= band < n_bands:
            raise SphxError(SPHX_ERR_ARG, "SPHX:Stats:band", f"band must be an integer in 0..{n_bands - 1}")
        m = self._channels()
        arrs = [np.zeros(m * n_bins) for _ in range(5)]
        ns, t0, t1 = np.zeros(m, dtype=np.int64), np.zeros(m), np.zeros(m)
        nb = C.c_int(0)
        self._call("flow_stats_read", C.c_int(int(band)), C.c_int(n_bins), C.byref(nb), *[ptr(a) for a in arrs],
                   ns.ctypes.data_as(C.POINTER(C.c_int64)), ptr(t0), ptr(t1))
        assert nb.value == n_bins, (nb.value, n_bins)
        out = []
        for k in range(m):
            d = {f: a[k * n_bins:(k + 1) * n_bins].copy() for f, a in zip(("count", "sum_ux", "sum_ux2", "sum_uy", "sum_uy2"), arrs)}
            d.update(n_samples=int(ns[k]), t_first=float(t0[k]), t_last=float(t1[k]))
            out.append(d)
        return self._each(out)

    # ---- step history (include/sphx.h sections 2d, 2f): wall shear, energy, bulk velocity, dt and vmax per step, recorded on the device ----
    def history_enable(self, every=1, capacity=65536, t_from=0.0):
        """Record every `every`-th completed step ending at t >= t_from into a device buffer of `capacity` records
        ((re)configures and empties it).  Records that find the buffer full are dropped and counted.  A batch: one config for
        all members, `capacity` records per member, each recorded on its own clock; n_members * capacity must not exceed
        1 << 24."""
        cfg = history_config(every, capacity, t_from, n_members=self._channels())
        self._call("history_enable", C.byref(cfg))

    def history_disable(self):
        self._call("history_disable")

    def history_records(self, drain=False):
        """-> (records [n x 8] in the order of HISTORY_FIELDS, n_dropped); drain empties the buffer after the copy.  A batch:
        one such pair per member, from one read of all members."""
        m = self._channels()
        n, dropped = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int64)

        def read(cap, rec, drain):  # the counts always; the records into rec [m x cap x 8] where there is one
            self._call("history_read", C.c_int(cap), ptr(rec), n.ctypes.data_as(C.POINTER(C.c_int)),
                       dropped.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int(1 if drain else 0))

        read(0, None, False)
        cap, want = max(int(n.max()), 1), n.copy()
        rec = np.zeros((m, cap, len(HISTORY_FIELDS)))
        read(cap, rec, drain)
        assert np.array_equal(n, want), (n, want)
        return self._each([(rec[k, :n[k]].copy(), int(dropped[k])) for k in range(m)])

    # ---- profile series (include/sphx.h sections 2j, 2k, 3a): the binned velocity profile, one record per sampled step ----
    def profile_series_enable(self, n_bins=0, every=1, capacity=4096, t_from=0.0, bands=()):
        """Record the flow statistics' sample of the state -- n_bins y-bins (0: the reference's max(20, round(DH/dp))) of the
        whole channel (band 0) and of up to two x-bands [(x_centre, half_width), ...] -- every `every`-th completed step ending
        at t >= t_from into a device buffer of `capacity` records ((re)configures and empties it).  Records that find the
        buffer full are dropped and counted.  A record is n_bands * n_bins * 5 doubles.  A batch: one config for all members,
        `capacity` records per member, each recorded on its own clock.  A slab of a ring: its own buffer, of PARTIAL samples
        over the particles it owns (slab.pool_ring_profile_series adds the ranks' up)."""
        p0 = self._params0()
        cfg = profile_series_config(p0, n_bins, every, capacity, t_from, bands, n_members=self._channels())
        self._call(self._series + "enable", C.byref(cfg))
        # (n_bins, n_bands incl. band 0) while the profile series is on
        self._profile_series = (int(cfg.n_bins) or max(20, int(np.floor(p0.DH / p0.dp + 0.5))), int(cfg.n_bands) + 1)

    def profile_series_disable(self):
        self._call(self._series + "disable")
        self._profile_series = None

    def _series_on(self):
        return _enabled(self._profile_series, "ProfileSeries", f"the profile series is not enabled on this {self._where}")

    def profile_series_sums(self, drain=False):
        """The raw series so far: step (int64) and t [n], the five STATS_FIELDS (count, sum_ux, sum_ux2, sum_uy, sum_uy2 of
        each sampled step) as [n, n_bands, n_bins] arrays, n_dropped and the bin centres y_mid; drain empties the buffer
        after the copy.  A batch: one such dict per member, from one read of all members.  A slab of a ring: its partial sums."""
        n_bins, n_bands = self._series_on()
        m = self._channels()
        n, dropped = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int64)
        nb, nbd = C.c_int(0), C.c_int(0)

        def read(cap, times, records, drain):
            self._call(self._series + "read", C.c_int(cap), ptr(times), ptr(records), C.byref(nb), C.byref(nbd),
                       n.ctypes.data_as(C.POINTER(C.c_int)), dropped.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int(1 if drain else 0))

        read(0, None, None, False)
        assert (nb.value, nbd.value) == (n_bins, n_bands), (nb.value, nbd.value, n_bins, n_bands)
        cap, want = max(int(n.max()), 1), n.copy()
        times, records = np.zeros((m, cap, 2)), np.zeros((m, cap, n_bands, n_bins, len(STATS_FIELDS)))
        read(cap, times, records, drain)
        assert np.array_equal(n, want), (n, want)
        DH = self._params0().DH
        return self._each([profile_series_dict(DH, times[k, :n[k]], records[k, :n[k]], int(dropped[k])) for k in range(m)])

    # ---- pair statistics (include/sphx.h sections 2l, 2m, 3a): what pair_dist_* of a context or a batch and pairs_part_* of a
    # slab (slab.HipSlabEngine) share -- the argument checks, the calls behind the stem and the read of the integer sums ----
    def _pairs_enable(self, n_bins, every, t_from, r_max, y_margin, with_walls, bands):
        p0 = self._params0()
        cfg = pair_dist_config(p0, n_bins, every, t_from, r_max, y_margin, with_walls, bands)
        self._call(self._pairs + "enable", C.byref(cfg))
        # (n_bins, n_bands incl. band 0, r_max in force) while the pair statistics are on
        self._pair_dist = (int(cfg.n_bins), int(cfg.n_bands) + 1, float(cfg.r_max) or 2.0 * p0.h)

    def _pairs_disable(self):
        self._call(self._pairs + "disable")
        self._pair_dist = None

    def _pairs_on(self):
        return _enabled(self._pair_dist, "PairDist", f"pair statistics are not enabled on this {self._where}")

    def _pairs_reset(self):
        self._pairs_on()
        self._call(self._pairs + "reset")

    def _pair_dist_band(self, band):
        n_bins, n_bands, r_max = self._pairs_on()
        if not _is_int(band) or not 0 <= band < n_bands:
            raise SphxError(SPHX_ERR_ARG, "SPHX:PairDist:band", f"band must be an integer in 0..{n_bands - 1}")
        m = self._channels()
        ff, fw = np.zeros((m, n_bins), dtype=np.int64), np.zeros((m, n_bins), dtype=np.int64)
        centres, ns = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
        r2, t0, t1 = np.zeros(m), np.zeros(m), np.zeros(m)
        nb = C.c_int(0)
        i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        self._call(self._pairs + "read", C.c_int(int(band)), C.c_int(n_bins), C.byref(nb), i64(ff), i64(fw), i64(centres), ptr(r2), i64(ns),
                   ptr(t0), ptr(t1))
        assert nb.value == n_bins, (nb.value, n_bins)
        r_edges = pair_edges(r_max, n_bins)[0]
        return [dict(r_edges=r_edges, ff=ff[k].copy(), fw=fw[k].copy(), centres=int(centres[k]), r2_min=float(r2[k]),
                     r_min=float(np.sqrt(r2[k])), n_samples=int(ns[k]), t_first=float(t0[k]), t_last=float(t1[k])) for k in range(m)]

    def _pair_dist_bands(self):
        """every band's sums: one list of band dicts per channel (a context or a slab: the list itself)"""
        n_bands = self._pairs_on()[1]
        per_band = [self._pair_dist_band(b) for b in range(n_bands)]
        return self._each([[per_band[b][k] for b in range(n_bands)] for k in range(self._channels())])

    # ---- gradient statistics (include/sphx.h sections 2n, 2o, 3a): what grad_stats_* of a context or a batch and grads_part_* of
    # a slab (slab.HipSlabEngine) share -- the argument checks, the calls behind the stem and the read of the sums ----
    def _grads_enable(self, n_bins, every, t_from, det_min, with_walls, bands):
        p0 = self._params0()
        cfg = grad_stats_config(p0, n_bins, every, t_from, det_min, with_walls, bands)
        self._call(self._grads + "enable", C.byref(cfg))
        # (n_bins, n_bands incl. band 0) while the gradient statistics are on
        self._grad_stats = (int(cfg.n_bins) or max(20, int(np.floor(p0.DH / p0.dp + 0.5))), int(cfg.n_bands) + 1)

    def _grads_disable(self):
        self._call(self._grads + "disable")
        self._grad_stats = None

    def _grads_on(self):
        return _enabled(getattr(self, "_grad_stats", None), "GradStats", f"gradient statistics are not enabled on this {self._where}")

    def _grads_reset(self):
        self._grads_on()
        self._call(self._grads + "reset")

    def _grad_stats_band(self, band):
        """one band's raw sums: one dict per channel"""
        n_bins, n_bands = self._grads_on()
        if not _is_int(band) or not 0 <= band < n_bands:
            raise SphxError(SPHX_ERR_ARG, "SPHX:GradStats:band", f"band must be an integer in 0..{n_bands - 1}")
        m = self._channels()
        sums = np.zeros((m, len(GRAD_FIELDS), n_bins))
        ns, t0, t1 = np.zeros(m, dtype=np.int64), np.zeros(m), np.zeros(m)
        nb = C.c_int(0)
        self._call(self._grads + "read", C.c_int(int(band)), C.c_int(n_bins), C.byref(nb), ptr(sums), ns.ctypes.data_as(C.POINTER(C.c_int64)),
                   ptr(t0), ptr(t1))
        assert nb.value == n_bins, (nb.value, n_bins)
        out = []
        for k in range(m):
            d = {f: sums[k, j].copy() for j, f in enumerate(GRAD_FIELDS)}
            d.update(n_samples=int(ns[k]), t_first=float(t0[k]), t_last=float(t1[k]))
            out.append(d)
        return out

    # ---- density statistics (include/sphx.h sections 2r, 2s, 3a): what dens_stats_* of a context or a batch and dens_part_* of a
    # slab (slab.HipSlabEngine) share -- the argument checks, the calls behind the stem and the read of the sums ----
    def _dens_enable(self, n_bins, every, t_from, n_hist, hist_range, delta_bound, bands):
        p0 = self._params0()
        cfg = dens_stats_config(p0, n_bins, every, t_from, n_hist, hist_range, delta_bound, bands)
        self._call(self._dens + "enable", C.byref(cfg))
        # (n_bins, n_bands incl. band 0, n_hist, hist_range) while the density statistics are on
        self._dens_stats = (int(cfg.n_bins) or max(20, int(np.floor(p0.DH / p0.dp + 0.5))), int(cfg.n_bands) + 1, int(cfg.n_hist),
                            float(cfg.hist_range))

    def _dens_disable(self):
        self._call(self._dens + "disable")
        self._dens_stats = None

    def _dens_on(self):
        return _enabled(getattr(self, "_dens_stats", None), "DensStats", f"density statistics are not enabled on this {self._where}")

    def _dens_reset(self):
        self._dens_on()
        self._call(self._dens + "reset")

    def _dens_stats_band(self, band):
        """one band's raw sums: one dict per channel"""
        n_bins, n_bands, n_hist, hist_range = self._dens_on()
        if not _is_int(band) or not 0 <= band < n_bands:
            raise SphxError(SPHX_ERR_ARG, "SPHX:DensStats:band", f"band must be an integer in 0..{n_bands - 1}")
        out = []
        for k in range(self._channels()):
            sums, hist = np.zeros((len(DENS_FIELDS), n_bins)), np.zeros(n_hist, dtype=np.int64)
            below, above, ns = C.c_int64(0), C.c_int64(0), C.c_int64(0)
            t0, t1, nb, nh = C.c_double(0.0), C.c_double(0.0), C.c_int(0), C.c_int(0)
            member = (C.c_int(k),) if self._many else ()
            self._call(self._dens + "read", *member, C.c_int(int(band)), C.c_int(n_bins), C.c_int(n_hist), C.byref(nb), C.byref(nh),
                       ptr(sums), hist.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(below), C.byref(above), C.byref(ns), C.byref(t0),
                       C.byref(t1))
            assert (nb.value, nh.value) == (n_bins, n_hist), (nb.value, nh.value, n_bins, n_hist)
            d = {f: sums[j].copy() for j, f in enumerate(DENS_FIELDS)}
            d.update(hist=hist, below=int(below.value), above=int(above.value), hist_range=hist_range, n_samples=int(ns.value),
                     t_first=float(t0.value), t_last=float(t1.value))
            out.append(d)
        return out


class _Stepped(_Sampled):
    """What a context and a batch bind alike on top of that: the handle's lifecycle, stepping, "sample now", the profiles
    and dicts made of the sums and records, and the field map."""

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            getattr(lib(), self._stem + "destroy")(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # advance, enqueue_steps and sync sit inside timed loops (bench.py): they go to the library without a helper in between
    def _status(self, name, *args):
        st = (SphxStatus * (self.n_members if self._many else 1))()
        check(getattr(lib(), self._stem + name)(self._h, *args, st))
        return [s.as_dict() for s in st] if self._many else st[0].as_dict()

    def advance(self, t_target, max_steps=0):
        return self._status("advance", C.c_double(t_target), C.c_int64(max_steps))

    def enqueue_steps(self, n_steps):
        check(getattr(lib(), self._stem + "enqueue_steps")(self._h, C.c_int64(n_steps)))

    def sync(self):
        return self._status("sync")

    def graph_stats(self) -> dict:
        a, b, g = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._call("graph_stats", C.byref(a), C.byref(b), C.byref(g))
        return dict(slots_replayed=a.value, slots_eager=b.value, graphs_captured=g.value)

    def _download(self, fields, *member):
        out, args = _field_buffers(self.n_total, fields)
        self._call("download", *member, *args)
        return out

    def _monitor(self, tau, pairs, *member):
        tb, tt, npairs = C.c_double(0), C.c_double(0), C.c_double(0)
        self._call("monitor", *member, C.byref(tb) if tau else None, C.byref(tt) if tau else None,
                   C.byref(npairs) if pairs else None)
        return tb.value, tt.value, npairs.value

    # ---- flow statistics (include/sphx.h sections 2a, 2c): "sample now" and the profile ----
    def flow_stats_sample(self):
        """Add one sample of the current state (what download() returns) now, whatever the gating; a batch: of every member."""
        self._stats_on()
        self._call("flow_stats_sample")

    def flow_stats(self, band=0):
        """Time-averaged profile of one band (profile.flow_stats_profile): y_mid, count, u_mean, u_std, uy_mean, uy_std,
        n_samples, t_first, t_last (+ the raw sums).  Empty bins give NaN means.  A batch: one such dict per member."""
        DH = self._params0().DH
        sums = self.flow_stats_sums(band)
        return [flow_stats_profile(DH, **s) for s in sums] if self._many else flow_stats_profile(DH, **sums)

    # ---- step history (include/sphx.h sections 2d, 2f): the records as a dict ----
    def history(self, drain=False):
        """The records so far as 1-D arrays step (int64), t, dt, vmax, tau_bottom, tau_top, kinetic_energy, u_bulk, plus
        n_dropped (history_dict); a batch: one such dict per member."""
        recs = self.history_records(drain)
        return [history_dict(*r) for r in recs] if self._many else history_dict(*recs)


    # ---- field map (include/sphx.h sections 2e, 2g): the velocity field on a regular grid in x and y, accumulated on the device ----
    def field_map_enable(self, nx=0, ny=0, every=1, t_from=0.0, with_walls=False):
        """Sample the state every `every`-th completed step ending at t >= t_from onto nx x ny nodes over [0, DL] x [0, DH],
        ends included (0: the reference's 2 round(DL/dp), 2 round(DH/dp)), by Shepard interpolation over the fluid
        particles -- and, with_walls, the wall particles with their wall velocity.  (Re)configures and zeroes the map.  A
        batch: one config and shape for all members, each sampled on its own clock; n_members * nx * ny must not exceed
        1 << 25."""
        cfg = field_map_config(nx, ny, every, t_from, with_walls, n_members=self._channels())
        shape = field_map_shape(self._params0(), nx, ny)
        self._call("field_map_enable", C.byref(cfg))
        self._field_map = shape  # (nx, ny) while the field map is on

    def field_map_disable(self):
        self._call("field_map_disable")
        self._field_map = None

    def _field_on(self):
        return _enabled(self._field_map, "Field", f"the field map is not enabled on this {self._where}")

    def field_map_reset(self):
        self._field_on()
        self._call("field_map_reset")

    def field_map_sample(self):
        """Add one sample of the current state (what download() returns) now, whatever the gating; a batch: of every member."""
        self._field_on()
        self._call("field_map_sample")

    def field_map_sums(self):
        """The raw planes count, sum_w, sum_ux, sum_uy, sum_ux2, sum_uy2 as [ny, nx] arrays, plus n_samples, t_first, t_last; a
        batch: one such dict per member, from one read of all members."""
        nx, ny = self._field_on()
        m, nn = self._channels(), nx * ny
        arrs = [np.zeros(m * nn) for _ in FIELD_MAP_PLANES]
        ns, t0, t1 = np.zeros(m, dtype=np.int64), np.zeros(m), np.zeros(m)
        gx, gy = C.c_int(0), C.c_int(0)
        self._call("field_map_read", C.c_int(nn), C.byref(gx), C.byref(gy), *[ptr(a) for a in arrs],
                   ns.ctypes.data_as(C.POINTER(C.c_int64)), ptr(t0), ptr(t1))
        assert (gx.value, gy.value) == (nx, ny), (gx.value, gy.value, nx, ny)
        out = []
        for k in range(m):
            # node (i, k) at i * ny + k: the rows of the [ny, nx] array are the y-levels
            d = {f: np.ascontiguousarray(a[k * nn:(k + 1) * nn].reshape(nx, ny).T) for f, a in zip(FIELD_MAP_PLANES, arrs)}
            d.update(n_samples=int(ns[k]), t_first=float(t0[k]), t_last=float(t1[k]))
            out.append(d)
        return self._each(out)

    def field_map(self):
        """The time-averaged map (profile.field_map_means): x [nx], y [ny] and count, weight, u_x, u_y, u_x_std, u_y_std as
        [ny, nx] arrays (NaN where count == 0), n_samples, t_first, t_last.  A batch: one such dict per member."""
        p0 = self._params0()
        sums = self.field_map_sums()
        return [field_map_means(p0.DL, p0.DH, **s) for s in sums] if self._many else field_map_means(p0.DL, p0.DH, **sums)

    # ---- point probes (include/sphx.h sections 2h, 2i): the flow at fixed points, one record per sampled step ----
    def probes_enable(self, points, every=1, capacity=65536, t_from=0.0, with_walls=False):
        """Record the Shepard sample of the state at the points [P, 2] (x any finite value, folded into [0, DL); 0 <= y <= DH)
        every `every`-th completed step ending at t >= t_from into a device buffer of `capacity` records ((re)configures and
        empties it).  Records that find the buffer full are dropped and counted.  A batch: one config and one set of points
        for all members, `capacity` records per member, each recorded on its own clock."""
        cfg, pts = probes_config(self._params0(), points, every, capacity, t_from, with_walls, n_members=self._channels())
        self._call("probes_enable", C.byref(cfg))
        self._probes = pts  # the folded points [P, 2] while the probes are on

    def probes_disable(self):
        self._call("probes_disable")
        self._probes = None

    def _probes_on(self):
        return _enabled(self._probes, "Probe", f"point probes are not enabled on this {self._where}")

    def probes_sample(self):
        """Append one record of the current state (what download() returns) now, whatever the gating; a batch: of every member."""
        self._probes_on()
        self._call("probes_sample")

    def probes(self, drain=False):
        """The series so far: points [P, 2] as folded, step (int64) and t [n], weight, u_x, u_y and rho [n, P] (velocities NaN
        and weight = rho = 0 where a point has no particle within 2h), n_dropped; drain empties the buffer after the copy.
        p0 * (rho / rho0 - 1) is the pressure of the summation density.  A batch: one such dict per member, from one read of
        all members."""
        pts = self._probes_on()
        m, P = self._channels(), len(pts)
        n, dropped, np_ = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int64), C.c_int(0)

        def read(cap, times, values, drain):
            self._call("probes_read", C.c_int(cap), ptr(times), ptr(values), C.byref(np_), n.ctypes.data_as(C.POINTER(C.c_int)),
                       dropped.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int(1 if drain else 0))

        read(0, None, None, False)
        assert np_.value == P, (np_.value, P)
        cap, want = max(int(n.max()), 1), n.copy()
        times, values = np.zeros((m, cap, 2)), np.zeros((m, cap, P, len(PROBE_FIELDS)))
        read(cap, times, values, drain)
        assert np.array_equal(n, want), (n, want)
        return self._each([probes_dict(pts, times[k, :n[k]], values[k, :n[k]], int(dropped[k])) for k in range(m)])

    # ---- particle tracers (include/sphx.h sections 2p, 2q): chosen fluid rows followed, one record per sampled step ----
    def tracers_enable(self, ids, every=1, capacity=65536, t_from=0.0):
        """Record x, y, u_x, u_y of the fluid rows `ids` (row numbers of download(), 0-based, any order, no duplicates) every
        `every`-th completed step ending at t >= t_from into a device buffer of `capacity` records ((re)configures and
        empties it).  Records that find the buffer full are dropped and counted.  A batch: one config and one id list for all
        members, `capacity` records per member, each recorded on its own clock."""
        cfg, ids = tracers_config(self.n_fluid, self.n_total, ids, every, capacity, t_from, n_members=self._channels())
        self._call("tracers_enable", C.byref(cfg))
        self._tracers = ids  # the ids [T] (int32) while the tracers are on

    def tracers_disable(self):
        self._call("tracers_disable")
        self._tracers = None

    def _tracers_on(self):
        return _enabled(getattr(self, "_tracers", None), "Tracers", f"particle tracers are not enabled on this {self._where}")

    def tracers_sample(self):
        """Append one record of the current state (what download() returns) now, whatever the gating; a batch: of every member."""
        self._tracers_on()
        self._call("tracers_sample")

    def tracers(self, drain=False):
        """The series so far: ids [T] as given, step (int64) and t [n], x, y, u_x and u_y [n, T] -- column k is ids[k], the values
        are the bits download() returns in that row -- n_dropped and n_missing (tracers no slot held: always 0); drain empties
        the buffer after the copy.  A batch: one such dict per member, from one read of all members."""
        ids = self._tracers_on()
        m, T = self._channels(), len(ids)
        n, dropped, missing = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
        nt_, got = C.c_int(0), np.zeros(T, dtype=np.int32)

        def read(cap, times, values, drain):
            self._call("tracers_read", C.c_int(cap), ptr(times), ptr(values), got.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nt_),
                       n.ctypes.data_as(C.POINTER(C.c_int)), dropped.ctypes.data_as(C.POINTER(C.c_int64)),
                       missing.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int(1 if drain else 0))

        read(0, None, None, False)
        assert nt_.value == T and np.array_equal(got, ids), (nt_.value, T)
        cap, want = max(int(n.max()), 1), n.copy()
        times, values = np.zeros((m, cap, 2)), np.zeros((m, cap, T, len(TRACER_FIELDS)))
        read(cap, times, values, drain)
        assert np.array_equal(n, want), (n, want)
        return self._each([tracers_dict(ids, times[k, :n[k]], values[k, :n[k]], int(dropped[k]), int(missing[k])) for k in range(m)])

    # ---- profile series (include/sphx.h sections 2j, 2k): "sample now" and the profiles ----
    def profile_series_sample(self):
        """Append one record of the current state (what download() returns) now, whatever the gating; a batch: of every member."""
        self._series_on()
        self._call("profile_series_sample")

    def profile_series(self, drain=False):
        """The series so far as profiles (profile.profile_series_profiles): step, t, y_mid and u_mean, u_std, uy_mean, uy_std,
        count as [n, n_bands, n_bins] arrays, NaN where a bin is empty, n_dropped.  A batch: one such dict per member."""
        DH = self._params0().DH
        sums = self.profile_series_sums(drain)
        return [profile_series_profiles(DH, s) for s in sums] if self._many else profile_series_profiles(DH, sums)

    # ---- pair statistics (include/sphx.h sections 2l, 2m): the pair-distance histogram of the fluid particles ----
    def pair_dist_enable(self, n_bins=64, every=1, t_from=0.0, r_max=0.0, y_margin=0.0, with_walls=False, bands=()):
        """Count, every `every`-th completed step ending at t >= t_from, the partners of every fluid particle with
        y_margin <= y <= DH - y_margin by distance, into n_bins uniform bins in r on [0, r_max) (r_max = 0: 2h; at most 2h): ff
        (fluid partners), with_walls: fw (wall partners), for the whole channel (band 0) and for the centres in up to two
        x-bands [(x_centre, half_width), ...].  Integer sums: exact, profile.pair_histogram gives the same counts.
        (Re)configures and zeroes the sums.  A batch: one config for all members, each sampled on its own clock."""
        self._pairs_enable(n_bins, every, t_from, r_max, y_margin, with_walls, bands)

    def pair_dist_disable(self):
        self._pairs_disable()

    def pair_dist_reset(self):
        self._pairs_reset()

    def pair_dist_sample(self):
        """Add one sample of the current state (what download() returns) now, whatever the gating; a batch: of every member."""
        self._pairs_on()
        self._call("pair_dist_sample")

    def pair_dist_sums(self):
        """The raw sums so far, one dict per band (band 0: the whole channel): r_edges [n_bins + 1], ff, fw [n_bins] (int64),
        centres, r2_min, r_min (+inf before any pair), n_samples, t_first, t_last.  A batch: one such list per member."""
        return self._pair_dist_bands()

    def pair_dist(self, band=0):
        """One band's sums with the figures of profile.pair_dist_profiles: r_mid, g, g_wall, n_neigh, r_min.  A batch: one such
        dict per member."""
        dp = self._params0().dp
        return self._each([dict(s, **pair_dist_profiles(s, dp)) for s in self._pair_dist_band(band)])

    # ---- gradient statistics (include/sphx.h sections 2n, 2o): the velocity gradient at the fluid particles, binned ----
    def grad_stats_enable(self, n_bins=0, every=1, t_from=0.0, det_min=0.05, with_walls=False, bands=()):
        """Estimate, every `every`-th completed step ending at t >= t_from, the velocity gradient G_ab = d u_a / d x_b at every
        fluid particle (profile.velocity_gradients) and add g_xx, g_xy, g_yx, g_yy, their squares, div^2 and vort^2 to n_bins
        y-bins (0: the reference's max(20, round(DH/dp))) of the whole channel (band 0) and of up to two x-bands
        [(x_centre, half_width), ...].  A particle with det M <= det_min or an estimate out of range is counted in `skipped`.
        with_walls: the wall particles are partners too, with the wall's velocity -- off by default, because they pull the
        estimate next to a wall towards the wall's velocity.  (Re)configures and zeroes the sums.  A batch: one config for all
        members, each sampled on its own clock."""
        self._grads_enable(n_bins, every, t_from, det_min, with_walls, bands)

    def grad_stats_disable(self):
        self._grads_disable()

    def grad_stats_reset(self):
        self._grads_reset()

    def grad_stats_sample(self):
        """Add one sample of the current state (what download() returns) now, whatever the gating; a batch: of every member."""
        self._grads_on()
        self._call("grad_stats_sample")

    def grad_stats_sums(self, band=0):
        """The raw sums of one band: the twelve profile.GRAD_FIELDS as [n_bins] arrays (count and skipped hold integers),
        n_samples, t_first, t_last; a batch: one such dict per member, from one read of all members."""
        return self._each(self._grad_stats_band(band))

    def grad_stats(self, band=0):
        """One band's profiles (profile.grad_stats_profiles): y_mid, count, skipped, the mean and standard deviation of each
        component (gxx_mean, gxx_std, ... gyy_std; gxy is the shear rate du_x/dy), div_rms, vort_mean, vort_rms, NaN where a bin
        is empty, plus the raw sums, n_samples, t_first, t_last.  A batch: one such dict per member."""
        DH = self._params0().DH
        sums = self.grad_stats_sums(band)
        per = [dict(s, **grad_stats_profiles(DH, s)) for s in (sums if self._many else [sums])]
        return self._each(per)

    # ---- density statistics (include/sphx.h sections 2r, 2s): the summation density at the fluid particles, binned ----
    def dens_stats_enable(self, n_bins=0, every=1, t_from=0.0, n_hist=64, hist_range=0.05, delta_bound=0.5, bands=()):
        """Re-sum, every `every`-th completed step ending at t >= t_from, the density the next step starts from at every fluid
        particle (profile.summation_density, the walls always in) and add delta = rho / rho0 - 1, its square, the volume defect
        rho0 / rho - 1 and the walls' share of rho / rho0 to n_bins y-bins (0: the reference's max(20, round(DH/dp))) of the
        whole channel (band 0) and of up to two x-bands [(x_centre, half_width), ...], with the extremes of delta per bin and
        per band a histogram of delta in n_hist bins on [-hist_range, hist_range).  A particle with |delta| > delta_bound is
        counted in `outliers`.  (Re)configures and zeroes the sums.  A batch: one config for all members, each sampled on its
        own clock."""
        self._dens_enable(n_bins, every, t_from, n_hist, hist_range, delta_bound, bands)

    def dens_stats_disable(self):
        self._dens_disable()

    def dens_stats_reset(self):
        self._dens_reset()

    def dens_stats_sample(self):
        """Add one sample of the current state (what download() returns) now, whatever the gating; a batch: of every member."""
        self._dens_on()
        self._call("dens_stats_sample")

    def dens_stats_sums(self, band=0):
        """The raw sums of one band: the eight profile.DENS_FIELDS as [n_bins] arrays (count and outliers hold integers; d_min /
        d_max are +inf / -inf in a bin without a particle), hist [n_hist] (int64), below, above, hist_range, n_samples, t_first,
        t_last; a batch: one such dict per member."""
        return self._each(self._dens_stats_band(band))

    def dens_stats(self, band=0):
        """One band's profiles (profile.dens_stats_profiles): y_mid, count, outliers, d_mean, d_std, d_min, d_max, p_mean, p_std,
        wall_mean, packing, NaN where a bin is empty, hist_centres and hist_density, plus the raw sums, n_samples, t_first,
        t_last.  A batch: one such dict per member, each with its own p0."""
        DH = self._params0().DH
        sums = self.dens_stats_sums(band)
        prms = self.params if self._many else [self.params]
        per = [dict(s, **dens_stats_profiles(DH, p.p0, s)) for p, s in zip(prms, sums if self._many else [sums])]
        return self._each(per)

    # ---- mode amplitudes (include/sphx.h sections 2t, 2u): the flow on the channel's modes, one record per sampled step ----
    def modes_enable(self, mx=4, ny=8, every=1, capacity=4096, t_from=0.0):
        """Record, every `every`-th completed step ending at t >= t_from, the sums of 1, u_x and u_y over the fluid particles
        times cos / sin(m 2 pi x / DL) cos / sin(n pi y / DH) for 0 <= m <= mx, 0 <= n <= ny (profile.mode_sums) into a
        device buffer of `capacity` records ((re)configures and empties it).  Records that find the buffer full are dropped
        and counted.  A record is (mx + 1) * (ny + 1) * 12 doubles.  A batch: one config for all members, `capacity` records
        per member, each recorded on its own clock."""
        cfg = modes_config(mx, ny, every, capacity, t_from, n_members=self._channels())
        self._call("modes_enable", C.byref(cfg))
        self._modes = (int(cfg.mx), int(cfg.ny))  # (mx, ny) while the mode amplitudes are on

    def modes_disable(self):
        self._call("modes_disable")
        self._modes = None

    def _modes_on(self):
        return _enabled(self._modes, "Modes", f"mode amplitudes are not enabled on this {self._where}")

    def modes_sample(self):
        """Append one record of the current state (what download() returns) now, whatever the gating; a batch: of every member."""
        self._modes_on()
        self._call("modes_sample")

    def modes(self, drain=False):
        """The records so far: step (int64) and t [n], the three MODE_FIELDS n, ux, uy as [n, mx + 1, ny + 1, 4] arrays (last
        axis: MODE_BASES cc, sc, cs, ss) and n_dropped; drain empties the buffer after the copy.  A batch: one such dict per
        member, from one read of all members."""
        mx, ny = self._modes_on()
        m = self._channels()
        n, dropped = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int64)
        gx, gy = C.c_int(0), C.c_int(0)

        def read(cap, times, records, drain):
            self._call("modes_read", C.c_int(cap), ptr(times), ptr(records), C.byref(gx), C.byref(gy),
                       n.ctypes.data_as(C.POINTER(C.c_int)), dropped.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int(1 if drain else 0))

        read(0, None, None, False)
        assert (gx.value, gy.value) == (mx, ny), (gx.value, gy.value, mx, ny)
        cap, want = max(int(n.max()), 1), n.copy()
        times = np.zeros((m, cap, 2))
        records = np.zeros((m, cap, mx + 1, ny + 1, len(MODE_FIELDS), len(MODE_BASES)))
        read(cap, times, records, drain)
        assert np.array_equal(n, want), (n, want)
        return self._each([modes_dict(times[k, :n[k]], records[k, :n[k]], int(dropped[k])) for k in range(m)])


class Batch(_Stepped):
    """M channels of one geometry stepped by the same launches (sphx_batch, include/sphx.h section 2b).

    prms: one parameter set per member (mu, c_f, p0, gravity_g, transport_coeff may differ; the geometry, t_end and the
    launch shape must not).  pos_list / vel_list / drho_list: the members' states, MEX layout as for Context; mass and
    wall_vel are shared.  transport_coeff may be a scalar or one value per member.  advance / sync, flow_stats_*,
    history_* and field_map_* are a context's for all members at once: one entry per member."""
    _stem, _where, _many = "sphx_batch_", "batch", True

    def __init__(self, prms, n_fluid, n_total, pos_list, vel_list, drho_list, mass, wall_vel, t0=0.0, step0=0,
                 t_end=None, transport_coeff=None, lanes_per_particle=0, steps_per_graph=0, rebuild_every=0,
                 skin_h=0.0, dynamic_rebin=0, dual_rate=0):
        self._h = C.c_void_p()
        prms = list(prms)
        m = len(prms)
        if m < 1:
            raise SphxError(SPHX_ERR_ARG, "SPHX:Batch:members", "a batch needs at least one member")
        self.n_members, self.n_fluid, self.n_total = m, int(n_fluid), int(n_total)
        nt = self.n_total
        tcs = _per_member(transport_coeff, m, "transport_coeff")
        self.params = [make_params(p, t_end, tc, lanes_per_particle, steps_per_graph, rebuild_every, skin_h,
                                   dynamic_rebin, dual_rate) for p, tc in zip(prms, tcs)]
        states = []
        for name, arrs, shape in (("pos", pos_list, (nt, 2)), ("vel", vel_list, (nt, 2)), ("drho_dt", drho_list, (nt,))):
            arrs = [f64(a) for a in arrs]
            if len(arrs) != m:
                raise SphxError(SPHX_ERR_ARG, "SPHX:Batch:members", f"{name}: {len(arrs)} arrays for {m} members")
            for k, a in enumerate(arrs):
                if a.shape != shape:
                    raise SphxError(SPHX_ERR_ARG, "SPHX:Batch:geometry",
                                    f"member {k}: {name} has shape {a.shape}, the batch's n_total asks for {shape}")
            # member blocks one after the other, each in MEX (column-major) layout
            states.append(np.concatenate([a.ravel(order="F") for a in arrs]))
        mass, wall_vel = f64(mass), f64(wall_vel)
        if mass.shape != (nt,) or wall_vel.shape != (nt, 2):
            raise SphxError(SPHX_ERR_ARG, "SPHX:Batch:geometry", "mass / wall_vel: shared arrays of n_total rows expected")
        self._flow_stats = None  # (n_bins, n_bands incl. band 0) while the flow statistics are on
        self._field_map = None   # (nx, ny) while the field map is on
        self._probes = None      # the folded points [P, 2] while the probes are on
        self._profile_series = None  # (n_bins, n_bands incl. band 0) while the profile series is on
        self._pair_dist = None   # (n_bins, n_bands incl. band 0, r_max) while the pair statistics are on
        self._grad_stats = None  # (n_bins, n_bands incl. band 0) while the gradient statistics are on
        self._tracers = None     # the ids [T] (int32) while the tracers are on
        self._dens_stats = None  # (n_bins, n_bands incl. band 0, n_hist, hist_range) while the density statistics are on
        self._modes = None       # (mx, ny) while the mode amplitudes are on
        arr = (SphxParams * m)(*self.params)
        check(lib().sphx_batch_create(C.byref(self._h), C.c_int(m), arr, C.c_int(n_fluid), C.c_int(n_total),
                                      ptr(states[0]), ptr(states[1]), ptr(states[2]), ptr(mass), ptr(wall_vel),
                                      C.c_double(t0), C.c_int64(step0)))

    @classmethod
    def from_parts(cls, prms, parts_list, **kw):
        """A batch of the particle sets parts_list (dicts of geometry.init_particles), one per member; mass and wall_vel are
        member 0's.  kw: the keywords of Batch(); an array given there (pos_list=, ..., mass=, wall_vel=) wins over the dicts'."""
        p0 = parts_list[0]
        states = [kw.pop(name, [pa[k] for pa in parts_list])
                  for name, k in (("pos_list", "pos"), ("vel_list", "vel"), ("drho_list", "drho_dt"))]
        return cls(prms, p0["n_fluid"], p0["n_total"], *states, kw.pop("mass", p0["mass"]),
                   kw.pop("wall_vel", p0["wall_vel"]), **kw)

    def download(self, member, fields=_FIELDS) -> dict:
        return self._download(fields, C.c_int(member))

    def monitor(self, member, tau=True, pairs=False):
        return self._monitor(tau, pairs, C.c_int(member))

    def info(self) -> dict:
        m, lpp, spg, k = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        skin, forced, realign = C.c_double(0.0), C.c_int64(0), C.c_int64(0)
        self._call("info", C.byref(m), C.byref(lpp), C.byref(spg), C.byref(k), C.byref(skin), C.byref(forced),
                   C.byref(realign))
        return dict(n_members=m.value, lanes_per_particle=lpp.value, steps_per_graph=spg.value, rebuild_every=k.value,
                    skin=skin.value, forced_rebuilds=forced.value, realignments=realign.value)


class Context(_Stepped):
    """Device-resident simulation state (sphx_ctx)."""
    _stem, _where = "sphx_ctx_", "context"

    def __init__(self, prm, n_fluid, n_total, pos, vel, drho_dt, mass, wall_vel, t0=0.0, step0=0,
                 t_end=None, transport_coeff=None, lanes_per_particle=0, steps_per_graph=0, rebuild_every=0,
                 skin_h=0.0, dynamic_rebin=0, dual_rate=0):
        self._h = C.c_void_p()
        self.n_fluid, self.n_total = int(n_fluid), int(n_total)
        self.params = make_params(prm, t_end, transport_coeff, lanes_per_particle, steps_per_graph, rebuild_every,
                                  skin_h, dynamic_rebin, dual_rate)
        pos, vel, wall_vel = f64(pos), f64(vel), f64(wall_vel)
        drho_dt, mass = f64(drho_dt), f64(mass)
        assert pos.shape == (n_total, 2) and vel.shape == (n_total, 2) and wall_vel.shape == (n_total, 2)
        assert drho_dt.shape == (n_total,) and mass.shape == (n_total,)
        self._flow_stats = None  # (n_bins, n_bands incl. band 0) while the flow statistics are on
        self._field_map = None   # (nx, ny) while the field map is on
        self._probes = None      # the folded points [P, 2] while the probes are on
        self._profile_series = None  # (n_bins, n_bands incl. band 0) while the profile series is on
        self._pair_dist = None   # (n_bins, n_bands incl. band 0, r_max) while the pair statistics are on
        self._grad_stats = None  # (n_bins, n_bands incl. band 0) while the gradient statistics are on
        self._tracers = None     # the ids [T] (int32) while the tracers are on
        self._dens_stats = None  # (n_bins, n_bands incl. band 0, n_hist, hist_range) while the density statistics are on
        self._modes = None       # (mx, ny) while the mode amplitudes are on
        check(lib().sphx_ctx_create(C.byref(self._h), C.byref(self.params), C.c_int(n_fluid), C.c_int(n_total),
                                    ptr(pos), ptr(vel), ptr(drho_dt), ptr(mass), ptr(wall_vel),
                                    C.c_double(t0), C.c_int64(step0)))

    @classmethod
    def from_parts(cls, prm, parts, **kw):
        """A context of the particle set parts (a dict of geometry.init_particles).  kw: the keywords of Context(); an array
        given there (pos=, vel=, drho_dt=, mass=, wall_vel=) wins over the dict's."""
        return cls(prm, parts["n_fluid"], parts["n_total"], *[kw.pop(k, parts[k]) for k in _STATE], **kw)

    def prepare_steps(self, n_steps):
        """Capture (without running) the graphs the next enqueue_steps(n_steps) / advance(max_steps=n_steps) replays."""
        self._call("prepare_steps", C.c_int64(n_steps))

    def download(self, fields=_FIELDS) -> dict:
        return self._download(fields)

    def monitor(self, tau=True, pairs=False):
        return self._monitor(tau, pairs)

    def neighbor_list(self):
        n = C.c_size_t(0)
        check(lib().sphx_ctx_neighbor_list(self._h, C.byref(n)))
        return _fetch_pairs(n.value)

    def info(self):
        a, b, c, d = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().sphx_ctx_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(n_fluid=a.value, n_wall=b.value, n_cell_x=c.value, n_cell_y=d.value)

    def grid_policy(self):
        a, b, c, d = C.c_int(0), C.c_double(0.0), C.c_int64(0), C.c_double(0.0)
        check(lib().sphx_ctx_grid_policy(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(rebuild_every=a.value, skin=b.value, forced_rebuilds=c.value, drift=d.value)

    def tuning(self):
        a, b = C.c_int(0), C.c_int(0)
        check(lib().sphx_ctx_tuning(self._h, C.byref(a), C.byref(b)))
        return dict(lanes_per_particle=a.value, steps_per_graph=b.value, block_size=self.block_size())

    def block_size(self) -> int:
        """Threads per workgroup of the compact step kernels (sphx_ctx_block_size); 256 with a library from before the choice."""
        f = getattr(lib(), "sphx_ctx_block_size", None)
        if f is None:
            return 256
        n = C.c_int(0)
        check(f(self._h, C.byref(n)))
        return n.value

    def schedule(self):
        """Launch schedule in force and the re-binnings carried out by step slots so far (sphx_ctx_schedule)."""
        a, b, d, r = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
        check(lib().sphx_ctx_schedule(self._h, C.byref(a), C.byref(b), C.byref(d), C.byref(r)))
        return dict(fuse_ea=a.value, tail_clock=b.value, dynamic=d.value, rebins=r.value)

    def kernel_forms(self):
        """Which forms of the passes the context runs (sphx_ctx_kernel_forms)."""
        v = [C.c_int(0) for _ in range(4)]
        check(lib().sphx_ctx_kernel_forms(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("walk_kernels", "lds_tiles", "tiles_abe", "coded_lists"), (bool(x.value) for x in v)))

    def substeps(self) -> int:
        """Inner sub-steps per step slot (1 = the reference's single-rate loop, see sphx_params.dual_rate)."""
        n = C.c_int(0)
        check(lib().sphx_ctx_substeps(self._h, C.byref(n)))
        return n.value

    def time_kernel(self, name, reps=200) -> float:
        ms = C.c_double(0.0)
        check(lib().sphx_ctx_time_kernel(self._h, name.encode(), C.c_int(reps), C.byref(ms)))
        return ms.value

    def profile_enable(self, on=True):
        check(lib().sphx_ctx_profile_enable(self._h, C.c_int(1 if on else 0)))

    def profile_read(self) -> dict:
        cap = 32
        names = (C.c_char_p * cap)()
        avg = (C.c_double * cap)()
        cnt = (C.c_int64 * cap)()
        n = C.c_int(0)
        check(lib().sphx_ctx_profile_read(self._h, C.c_int(cap), names, avg, cnt, C.byref(n)))
        return {names[k].decode(): dict(avg_ms=avg[k], launches=cnt[k]) for k in range(min(n.value, cap))}


def _enabled(state, stem, text):
    """state, what a sampler's enable left in the wrapper; SPHX:<stem>:disabled while it is off (None)."""
    if state is None:
        raise SphxError(SPHX_ERR_STATE, f"SPHX:{stem}:disabled", text)
    return state


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _config_error(stem):
    """bad(msg) -> the SPHX:<stem>:config error of a validator."""
    return lambda msg: SphxError(SPHX_ERR_ARG, f"SPHX:{stem}:config", msg)


def _check_every(every, bad) -> int:
    if not _is_int(every) or every < 1:
        raise bad("every must be an integer >= 1")
    return int(every)


def _check_t_from(t_from, bad, finite=False, not_a_number="t_from must be a number") -> float:
    """t_from as a float: never NaN; finite: not infinite either (the history's records carry it)."""
    try:
        t_from = float(t_from)
    except (TypeError, ValueError):
        raise bad(not_a_number) from None
    if finite and not np.isfinite(t_from):
        raise bad("t_from must be finite")
    if np.isnan(t_from):
        raise bad("t_from must not be NaN")
    return t_from


def flow_stats_config(n_bins=0, every=1, t_from=0.0, bands=()) -> SphxFlowStatsConfig:
    """Checked sphx_flow_stats_config; raises SphxError(SPHX:Stats:config) before anything reaches the device."""
    bad = _config_error("Stats")
    not_numbers = "t_from must be a number and bands a sequence of (x_centre, half_width) pairs"
    if not _is_int(n_bins) or n_bins < 0:
        raise bad("n_bins must be an integer >= 0 (0 = the reference's profile bins)")
    every = _check_every(every, bad)
    try:
        bands = [tuple(float(v) for v in b) for b in bands]
    except (TypeError, ValueError):
        raise bad(not_numbers) from None
    t_from = _check_t_from(t_from, bad, not_a_number=not_numbers)
    if len(bands) > 2 or any(len(b) != 2 for b in bands):
        raise bad("at most two bands, each (x_centre, half_width)")
    if any(not (np.isfinite(x) and np.isfinite(hw) and hw >= 0.0) for x, hw in bands):
        raise bad("band centres must be finite and half-widths finite and >= 0")
    if n_bins * (len(bands) + 1) > 1536:
        raise bad("n_bins * (number of bands + 1) must not exceed 1536")
    cfg = SphxFlowStatsConfig(n_bins=int(n_bins), every=every, t_from=t_from, n_bands=len(bands))
    for k, (x, hw) in enumerate(bands):
        cfg.band_x[k], cfg.band_hw[k] = x, hw
    return cfg


def history_config(every=1, capacity=65536, t_from=0.0, n_members=1) -> SphxHistoryConfig:
    """Checked sphx_history_config; raises SphxError(SPHX:History:config) before anything reaches the device.  n_members:
    the channels that get `capacity` records each (a batch's members)."""
    bad = _config_error("History")
    every = _check_every(every, bad)
    if not _is_int(capacity) or not 1 <= capacity <= 1 << 22:
        raise bad("capacity must be an integer in 1 .. 1 << 22")
    if n_members * capacity > 1 << 24:
        raise bad("n_members * capacity must not exceed 1 << 24 records")
    return SphxHistoryConfig(every=every, capacity=int(capacity), t_from=_check_t_from(t_from, bad, finite=True))


def field_map_shape(prm, nx=0, ny=0):
    """(nx, ny) of a field map on a channel with parameters prm: 0 = the reference's 2 round(DL/dp), 2 round(DH/dp)
    (SPH_Poiseuille_postprocess.m:185-186)."""
    return (int(nx) or 2 * int(np.floor(prm.DL / prm.dp + 0.5)), int(ny) or 2 * int(np.floor(prm.DH / prm.dp + 0.5)))


def field_map_config(nx=0, ny=0, every=1, t_from=0.0, with_walls=False, n_members=1) -> SphxFieldMapConfig:
    """Checked sphx_field_map_config; raises SphxError(SPHX:Field:config) before anything reaches the device.  n_members: the
    channels that get nx x ny nodes each (a batch's members)."""
    bad = _config_error("Field")
    for name, v in (("nx", nx), ("ny", ny)):
        if not _is_int(v) or v < 0 or v == 1:
            raise bad(f"{name} must be an integer >= 2, or 0 for the reference's shape")
    if n_members * nx * ny > 1 << 25:
        raise bad(("n_members * " if n_members > 1 else "") + "nx * ny must not exceed 1 << 25 nodes")
    every = _check_every(every, bad)
    t_from = _check_t_from(t_from, bad)
    if not (isinstance(with_walls, (bool, np.bool_)) or (_is_int(with_walls) and with_walls in (0, 1))):
        raise bad("with_walls must be a bool (or 0 / 1)")
    return SphxFieldMapConfig(nx=int(nx), ny=int(ny), every=every, with_walls=int(with_walls), t_from=t_from)


def probes_fold(x, DL):
    """x folded into [0, DL) as the library folds it: x - floor(x / DL) * DL, and 0 where rounding lands on DL."""
    x = np.asarray(x, dtype=np.float64)
    f = x - np.floor(x / DL) * DL
    return np.where((f >= 0.0) & (f < DL), f, 0.0)


def probes_config(prm, points, every=1, capacity=65536, t_from=0.0, with_walls=False, n_members=1):
    """Checked sphx_probes_config for channels with parameters prm, and the folded points [P, 2] it points to (keep them
    alive through the call); raises SphxError(SPHX:Probe:config) before anything reaches the device.  n_members: the
    channels that get `capacity` records each (a batch's members)."""
    bad = _config_error("Probe")
    if points is None:
        raise bad("points must not be None")
    try:
        pts = np.array(points, dtype=np.float64)
    except (TypeError, ValueError):
        raise bad("points must be an array of (x, y) pairs") from None
    if pts.ndim != 2 or pts.shape[1] != 2:
        raise bad("points must be an array of (x, y) pairs, shape [P, 2]")
    if not 1 <= len(pts) <= PROBE_MAX_POINTS:
        raise bad(f"the number of points must be 1 .. {PROBE_MAX_POINTS}")
    if not np.all(np.isfinite(pts)):
        raise bad("the coordinates of a point must be finite")
    if np.any(pts[:, 1] < 0.0) or np.any(pts[:, 1] > prm.DH):
        raise bad("the y of a point must lie in [0, DH]")
    every = _check_every(every, bad)
    if not _is_int(capacity) or capacity < 1 or capacity >= 1 << 31:
        raise bad("capacity must be an integer >= 1")
    if n_members * capacity * len(pts) * len(PROBE_FIELDS) > 1 << 27:
        raise bad(("n_members * " if n_members > 1 else "") + "capacity * n_points * 4 must not exceed 1 << 27 doubles")
    t_from = _check_t_from(t_from, bad, finite=True)
    if not (isinstance(with_walls, (bool, np.bool_)) or (_is_int(with_walls) and with_walls in (0, 1))):
        raise bad("with_walls must be a bool (or 0 / 1)")
    pts = np.ascontiguousarray(np.column_stack([probes_fold(pts[:, 0], prm.DL), pts[:, 1]]))
    cfg = SphxProbesConfig(n_points=len(pts), every=every, capacity=int(capacity), with_walls=int(with_walls), t_from=t_from,
                           points=ptr(pts))
    return cfg, pts


def tracers_config(n_fluid, n_total, ids, every=1, capacity=65536, t_from=0.0, n_members=1):
    """Checked sphx_tracers_config for channels of n_fluid fluid rows among n_total, and the ids [T] (int32) it points to (keep
    them alive through the call); raises SphxError(SPHX:Tracers:config) before anything reaches the device.  n_members: the
    channels that get `capacity` records each (a batch's members)."""
    bad = _config_error("Tracers")
    if ids is None:
        raise bad("ids must not be None")
    try:
        raw = np.array(ids)
    except (TypeError, ValueError):
        raise bad("ids must be a list of row numbers") from None
    if raw.ndim != 1 or raw.dtype == np.bool_ or not (np.issubdtype(raw.dtype, np.integer) or raw.size == 0):
        raise bad("ids must be a one-dimensional list of integer row numbers")
    if not 1 <= raw.size <= n_fluid:
        raise bad("the number of tracers must be 1 .. n_fluid")
    raw = raw.astype(np.int64)
    if np.any((raw >= n_fluid) & (raw < n_total)):
        raise bad("a tracer must be a fluid row: rows n_fluid .. n_total - 1 are wall particles")
    if np.any(raw < 0) or np.any(raw >= n_fluid):
        raise bad("a tracer id must be a row number in 0 .. n_fluid - 1")
    if len(np.unique(raw)) != raw.size:
        raise bad("a row is listed twice")
    every = _check_every(every, bad)
    if not _is_int(capacity) or capacity < 1 or capacity >= 1 << 31:
        raise bad("capacity must be an integer >= 1")
    if n_members * capacity * raw.size * len(TRACER_FIELDS) > 1 << 27:
        raise bad(("n_members * " if n_members > 1 else "") + "capacity * n_tracers * 4 must not exceed 1 << 27 doubles")
    t_from = _check_t_from(t_from, bad, finite=True)
    out = np.ascontiguousarray(raw, dtype=np.int32)
    cfg = SphxTracersConfig(n_tracers=len(out), every=every, capacity=int(capacity), t_from=t_from,
                            ids=out.ctypes.data_as(C.POINTER(C.c_int32)))
    return cfg, out


def tracers_dict(ids, times, values, n_dropped=0, n_missing=0) -> dict:
    """times [n, 2] and values [n, T, 4] -> ids, step (int64), t [n] and one [n, T] array per TRACER_FIELDS, plus n_dropped and
    n_missing."""
    times = np.asarray(times, dtype=np.float64).reshape(-1, 2)
    ids = np.array(ids, dtype=np.int32).reshape(-1)
    values = np.asarray(values, dtype=np.float64).reshape(len(times), len(ids), len(TRACER_FIELDS))
    out = dict(ids=ids, step=times[:, 0].astype(np.int64), t=np.ascontiguousarray(times[:, 1]))
    out.update({k: np.ascontiguousarray(values[:, :, j]) for j, k in enumerate(TRACER_FIELDS)})
    out.update(n_dropped=int(n_dropped), n_missing=int(n_missing))
    return out


def profile_series_config(prm, n_bins=0, every=1, capacity=4096, t_from=0.0, bands=(), n_members=1) -> SphxProfileSeriesConfig:
    """Checked sphx_profile_series_config for channels with parameters prm: bins, bands, every and t_from by the checks of
    flow_stats_config, the record buffer by those of the probes; raises SphxError(SPHX:ProfileSeries:config) before anything
    reaches the device.  n_members: the channels that get `capacity` records each (a batch's members)."""
    bad = _config_error("ProfileSeries")
    try:
        f = flow_stats_config(n_bins, every, t_from, bands)
    except SphxError as e:
        raise bad(e.message) from None
    if not _is_int(capacity) or capacity < 1 or capacity >= 1 << 31:
        raise bad("capacity must be an integer >= 1")
    bins = int(f.n_bins) or max(20, int(np.floor(prm.DH / prm.dp + 0.5)))
    if bins * (int(f.n_bands) + 1) > 1536:
        raise bad("n_bins * (number of bands + 1) must not exceed 1536")
    if n_members * capacity * (int(f.n_bands) + 1) * bins * len(STATS_FIELDS) > 1 << 27:
        raise bad(("n_members * " if n_members > 1 else "") + "capacity * (n_bands + 1) * n_bins * 5 must not exceed 1 << 27 doubles")
    cfg = SphxProfileSeriesConfig(n_bins=int(f.n_bins), every=int(f.every), capacity=int(capacity), t_from=float(f.t_from),
                                  n_bands=int(f.n_bands))
    for k in range(2):
        cfg.band_x[k], cfg.band_hw[k] = f.band_x[k], f.band_hw[k]
    return cfg


def pair_dist_config(prm, n_bins=64, every=1, t_from=0.0, r_max=0.0, y_margin=0.0, with_walls=False, bands=()) -> SphxPairDistConfig:
    """Checked sphx_pair_dist_config for channels with parameters prm; raises SphxError(SPHX:PairDist:config) before anything
    reaches the device.  every, t_from and the bands by the checks of flow_stats_config."""
    bad = _config_error("PairDist")
    if not _is_int(n_bins) or not 1 <= n_bins <= PAIR_DIST_MAX_BINS:
        raise bad("n_bins must be an integer in 1..1024")
    try:
        f = flow_stats_config(0, every, t_from, bands)
        r_max, y_margin = float(r_max), float(y_margin)
    except SphxError as e:
        raise bad(e.message) from None
    except (TypeError, ValueError):
        raise bad("r_max and y_margin must be numbers") from None
    if not (np.isfinite(r_max) and 0.0 <= r_max <= 2.0 * prm.h):
        raise bad("r_max must be 0 (= 2h) or 0 < r_max <= 2h: beyond 2h the sweep of the three cell columns is not complete")
    if not (np.isfinite(y_margin) and y_margin >= 0.0):
        raise bad("y_margin must be finite and >= 0")
    if not isinstance(with_walls, (bool, np.bool_)) and with_walls not in (0, 1):
        raise bad("with_walls must be a bool")
    cfg = SphxPairDistConfig(n_bins=int(n_bins), every=int(f.every), t_from=float(f.t_from), r_max=r_max, y_margin=y_margin,
                             with_walls=1 if with_walls else 0, n_bands=int(f.n_bands))
    for k in range(2):
        cfg.band_x[k], cfg.band_hw[k] = f.band_x[k], f.band_hw[k]
    return cfg


def grad_stats_config(prm, n_bins=0, every=1, t_from=0.0, det_min=0.05, with_walls=False, bands=()) -> SphxGradStatsConfig:
    """Checked sphx_grad_stats_config for channels with parameters prm; raises SphxError(SPHX:GradStats:config) before anything
    reaches the device.  n_bins, every, t_from and the bands by the checks of flow_stats_config."""
    bad = _config_error("GradStats")
    try:
        f = flow_stats_config(n_bins, every, t_from, bands)
        det_min = float(det_min)
    except SphxError as e:
        raise bad(e.message) from None
    except (TypeError, ValueError):
        raise bad("det_min must be a number") from None
    if not (np.isfinite(det_min) and det_min >= 0.0):
        raise bad("det_min must be finite and >= 0")
    if not isinstance(with_walls, (bool, np.bool_)) and with_walls not in (0, 1):
        raise bad("with_walls must be a bool")
    bins = int(f.n_bins) or max(20, int(np.floor(prm.DH / prm.dp + 0.5)))
    if bins * (int(f.n_bands) + 1) > GRAD_MAX_BINS:
        raise bad("n_bins * (number of bands + 1) must not exceed 640")
    cfg = SphxGradStatsConfig(n_bins=int(f.n_bins), every=int(f.every), t_from=float(f.t_from), det_min=det_min,
                              with_walls=1 if with_walls else 0, n_bands=int(f.n_bands))
    for k in range(2):
        cfg.band_x[k], cfg.band_hw[k] = f.band_x[k], f.band_hw[k]
    return cfg


def dens_stats_config(prm, n_bins=0, every=1, t_from=0.0, n_hist=64, hist_range=0.05, delta_bound=0.5, bands=()) -> SphxDensStatsConfig:
    """Checked sphx_dens_stats_config for channels with parameters prm; raises SphxError(SPHX:DensStats:config) before anything
    reaches the device.  n_bins, every, t_from and the bands by the checks of flow_stats_config."""
    bad = _config_error("DensStats")
    try:
        f = flow_stats_config(n_bins, every, t_from, bands)
        hist_range, delta_bound = float(hist_range), float(delta_bound)
    except SphxError as e:
        raise bad(e.message) from None
    except (TypeError, ValueError):
        raise bad("hist_range and delta_bound must be numbers") from None
    if not _is_int(n_hist) or not 1 <= n_hist <= DENS_MAX_HIST:
        raise bad("n_hist must be an integer in 1..1024")
    if not 0.0 < delta_bound <= 0.5:  # (a NaN fails)
        raise bad("delta_bound must be in (0, 0.5]")
    if not 0.0 < hist_range <= delta_bound:
        raise bad("hist_range must be in (0, delta_bound]")
    bins = int(f.n_bins) or max(20, int(np.floor(prm.DH / prm.dp + 0.5)))
    if (int(f.n_bands) + 1) * (8 * bins + int(n_hist) + 2) > DENS_MAX_WORDS:
        raise bad("(number of bands + 1) * (8 * n_bins + n_hist + 2) must not exceed 7680")
    cfg = SphxDensStatsConfig(n_bins=int(f.n_bins), every=int(f.every), t_from=float(f.t_from), n_hist=int(n_hist), n_bands=int(f.n_bands),
                              hist_range=hist_range, delta_bound=delta_bound)
    for k in range(2):
        cfg.band_x[k], cfg.band_hw[k] = f.band_x[k], f.band_hw[k]
    return cfg


def modes_config(mx=4, ny=8, every=1, capacity=4096, t_from=0.0, n_members=1) -> SphxModesConfig:
    """Checked sphx_modes_config; raises SphxError(SPHX:Modes:config) before anything reaches the device.  n_members: the
    channels that get `capacity` records each (a batch's members)."""
    bad = _config_error("Modes")
    for name, v in (("mx", mx), ("ny", ny)):
        if not _is_int(v) or not 0 <= v <= MODES_MAX:
            raise bad(f"{name} must be an integer in 0..16")
    try:
        f = flow_stats_config(0, every, t_from, ())
    except SphxError as e:
        raise bad(e.message) from None
    if not _is_int(capacity) or capacity < 1 or capacity >= 1 << 31:
        raise bad("capacity must be an integer >= 1")
    if n_members * capacity * (mx + 1) * (ny + 1) * len(MODE_FIELDS) * len(MODE_BASES) > 1 << 27:
        raise bad(("n_members * " if n_members > 1 else "") + "capacity * (mx + 1) * (ny + 1) * 12 must not exceed 1 << 27 doubles")
    return SphxModesConfig(mx=int(mx), ny=int(ny), every=int(f.every), capacity=int(capacity), t_from=float(f.t_from))


def modes_dict(times, records, n_dropped=0) -> dict:
    """times [n, 2] and records [n, mx + 1, ny + 1, 3, 4] -> step (int64), t [n], one [n, mx + 1, ny + 1, 4] array per
    MODE_FIELDS (last axis: MODE_BASES) and n_dropped."""
    times = np.asarray(times, dtype=np.float64).reshape(-1, 2)
    records = np.asarray(records, dtype=np.float64)
    assert records.ndim == 5 and records.shape[0] == len(times) and records.shape[3:] == (len(MODE_FIELDS), len(MODE_BASES)), records.shape
    out = dict(step=times[:, 0].astype(np.int64), t=np.ascontiguousarray(times[:, 1]))
    out.update({k: np.ascontiguousarray(records[:, :, :, j, :]) for j, k in enumerate(MODE_FIELDS)})
    out["n_dropped"] = int(n_dropped)
    return out


def profile_series_dict(DH, times, records, n_dropped=0) -> dict:
    """times [n, 2] and records [n, n_bands, n_bins, 5] -> step (int64), t [n], one [n, n_bands, n_bins] array per STATS_FIELDS,
    n_dropped and y_mid [n_bins], the bin centres of profile.flow_stats_profile."""
    times = np.asarray(times, dtype=np.float64).reshape(-1, 2)
    records = np.asarray(records, dtype=np.float64)
    assert records.ndim == 4 and records.shape[0] == len(times) and records.shape[3] == len(STATS_FIELDS), records.shape
    edges = np.linspace(0.0, DH, records.shape[2] + 1)
    out = dict(step=times[:, 0].astype(np.int64), t=np.ascontiguousarray(times[:, 1]))
    out.update({k: np.ascontiguousarray(records[:, :, :, j]) for j, k in enumerate(STATS_FIELDS)})
    out.update(n_dropped=int(n_dropped), y_mid=0.5 * (edges[:-1] + edges[1:]))
    return out


def probes_dict(points, times, values, n_dropped=0) -> dict:
    """times [n, 2] and values [n, P, 4] -> points, step (int64), t [n] and one [n, P] array per PROBE_FIELDS, plus n_dropped."""
    times = np.asarray(times, dtype=np.float64).reshape(-1, 2)
    points = np.array(points, dtype=np.float64).reshape(-1, 2)
    values = np.asarray(values, dtype=np.float64).reshape(len(times), len(points), len(PROBE_FIELDS))
    out = dict(points=points, step=times[:, 0].astype(np.int64), t=np.ascontiguousarray(times[:, 1]))
    out.update({k: np.ascontiguousarray(values[:, :, j]) for j, k in enumerate(PROBE_FIELDS)})
    out["n_dropped"] = int(n_dropped)
    return out


def history_dict(records, n_dropped=0) -> dict:
    """Records [n x 8] -> {field: 1-D array} in the order of HISTORY_FIELDS (step as int64) plus n_dropped."""
    records = np.asarray(records, dtype=np.float64).reshape(-1, len(HISTORY_FIELDS))
    out = {k: np.ascontiguousarray(records[:, j]) for j, k in enumerate(HISTORY_FIELDS)}
    out["step"] = out["step"].astype(np.int64)
    out["n_dropped"] = int(n_dropped)
    return out


def _fetch_pairs(n):
    cols = [np.zeros(max(n, 1)) for _ in range(7)]
    check(lib().sphx_neighbor_fetch(*[ptr(c) for c in cols], C.c_size_t(max(n, 1))))
    return tuple(c[:n] for c in cols)


def neighbor_search(pos, n_fluid, n_total, h, DL):
    pos = f64(pos)
    n = C.c_size_t(0)
    check(lib().sphx_neighbor_search(ptr(pos), C.c_int(n_fluid), C.c_int(n_total), C.c_double(h), C.c_double(DL),
                                     C.byref(n)))
    return _fetch_pairs(n.value)
