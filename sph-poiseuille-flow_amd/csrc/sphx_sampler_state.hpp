// sphx_sampler_state.hpp -- host state of the slot samplers ("Slot samplers"), part of the
// sphx_resident.hip translation unit: what sphx_ctx holds of each.  Launches, lifecycle and entry points: sphx_samplers.hpp.
#pragma once
#include "sphx_common.hpp"
#include "sphx_flow_stats.hpp"
#include "sphx_history.hpp"
#include "sphx_field_map.hpp"
#include "sphx_probes.hpp"
#include "sphx_profile_series.hpp"
#include "sphx_pair_dist.hpp"
#include "sphx_grad_stats.hpp"
#include "sphx_tracers.hpp"
#include "sphx_dens_stats.hpp"
#include "sphx_modes.hpp"

struct sphx_ctx;

namespace sphx {

// Flow statistics (sphx_ctx_flow_stats_*, sphx_batch_flow_stats_*; sphx_flow_stats.hpp) of a context or of the M members of
// a batch: one configuration, running sums and heads in M blocks (member m's sums at m * block(), its head at m).
struct FlowStats {
    bool on = false;
    int members = 1;
    sphx_flow_stats_config cfg{};
    int n_bins = 0, n_bands = 1;  // (n_bands counts band 0)
    DevBuf<unsigned long long> isum;
    DevBuf<double> dsum;
    DevBuf<FlowStatsHead> head;

    size_t row() const { return (size_t)n_bins * kStatsFields; }  // the sums of one band ...
    size_t block() const { return (size_t)n_bands * row(); }      // ... and of one member
    size_t shmem() const { return block() * sizeof(unsigned long long); }  // the LDS counters of a workgroup

    void configure(const sphx_params &prm, const sphx_flow_stats_config *cfg);
    void alloc(const FlowStats &checked, int M);
    void zero(hipStream_t st) { isum.zero(st); dsum.zero(st); head.zero(st); }
    void release() { isum.release(); dsum.release(); head.release(); }
    void read(hipStream_t st, int band, int stride, bool sums, double *const out[kStatsFields], int64_t *n_samples, double *t_first,
              double *t_last) const;
};

// Step history (sphx_ctx_history_*, sphx_batch_history_*; sphx_history.hpp) of a context or of the M members of a batch: one
// configuration, member m's records at m * cfg.capacity * kHistoryFields, its partials at m * kHistoryMaxBlocks *
// kHistorySums, its head at m.
struct History {
    bool on = false;
    int members = 1;
    sphx_history_config cfg{};
    DevBuf<double> records, part;
    DevBuf<HistoryHead> head;

    static void check(const sphx_history_config *cfg, int M);
    void alloc(const sphx_history_config &checked, int M);
    void zero(hipStream_t st) { head.zero(st); }  // (the counters: records beyond n_records are never read)
    void release() { records.release(); part.release(); head.release(); }
    void read(hipStream_t st, int capacity, double *records, int *n_records, int64_t *n_dropped, bool drain);
};

// Velocity-field map (sphx_ctx_field_map_*, sphx_batch_field_map_*; sphx_field_map.hpp) of a context or of the M members of a
// batch: one configuration and shape, member m's six planes at m * block(), its head at m.  Of a slab of a ring
// (sphx_slab_field_map_*): nx x ny is the ring's grid, the planes hold the block of node columns i_lo <= i < i_hi the slab owns.
struct FieldMap {
    bool on = false;
    int members = 1;
    sphx_field_map_config cfg{};
    int nx = 0, ny = 0;  // the shape in force (cfg.nx / cfg.ny = 0: the reference's)
    bool part = false;   // a slab's: the planes are those of the columns [i_lo, i_hi) only (possibly none)
    int i_lo = 0, i_hi = 0;
    DevBuf<double> planes;
    DevBuf<FieldMapHead> head;

    int cols() const { return part ? i_hi - i_lo : nx;  }  // node columns held
    size_t nodes() const { return (size_t)cols() * (size_t)ny; }
    size_t block() const { return nodes() * kFieldPlanes; }  // the planes of one member
    void check(const sphx_params &prm, const sphx_field_map_config *cfg, int M);
    void alloc(const FieldMap &checked, int M);
    void zero(hipStream_t st) { planes.zero(st); head.zero(st); }
    void release() { planes.release(); head.release(); }
    void read(hipStream_t st, int stride, double *const out[kFieldPlanes], int64_t *n_samples, double *t_first, double *t_last) const;
};

// Point probes (sphx_ctx_probes_*, sphx_batch_probes_*; sphx_probes.hpp) of a context or of the M members of a batch: one
// configuration and one set of points, member m's times at m * cfg.capacity * 2, its values at m * cfg.capacity * row(), its
// head at m.  Of a slab of a ring (sphx_slab_probes_*): cfg and folded are the ring's list, the same on every rank; the device
// holds the probes the slab owns -- those of `index`, in the ring's order -- and their values.
struct Probes {
    bool on = false;
    int members = 1;
    sphx_probes_config cfg{};     // (cfg.points: nullptr -- the points are copied)
    std::vector<double> folded;   // [n_points][2]: x folded into [0, DL), y
    bool part = false;            // a slab's: points / values are those of the probes of `index` only (possibly none)
    std::vector<int> index;       // [n_owned] positions of the owned probes in the ring's list, ascending
    DevBuf<double2> points;
    DevBuf<double> times, values;
    DevBuf<ProbeHead> head;

    int held() const { return part ? (int)index.size() : cfg.n_points; }  // probes on the device
    size_t row() const { return (size_t)held() * kProbeFields; }          // the values of one record
    void check(const sphx_params &prm, const sphx_probes_config *cfg, int M);
    void alloc(const Probes &checked, int M, hipStream_t st);
    void zero(hipStream_t st) { head.zero(st); }  // (the counters: records beyond n_records are never read)
    void release() { points.release(); times.release(); values.release(); head.release(); }
    void read(hipStream_t st, int capacity, double *times, double *values, int *n_records, int64_t *n_dropped, bool drain);
};

// Profile series (sphx_ctx_profile_series_*, sphx_batch_profile_series_*; sphx_profile_series.hpp) of a context or of the M
// members of a batch: one configuration, bins and bands as FlowStats has them, member m's int64 sums of the sample in flight
// at m * block(), its times at m * cfg.capacity * 2, its records at m * cfg.capacity * block(), its head at m.
struct ProfileSeries {
    bool on = false;
    int members = 1;
    sphx_profile_series_config cfg{};
    int n_bins = 0, n_bands = 1;  // (n_bands counts band 0)
    DevBuf<unsigned long long> isum;
    DevBuf<double> times, records;
    DevBuf<ProfileSeriesHead> head;

    size_t block() const { return (size_t)n_bands * (size_t)n_bins * kStatsFields; }  // the doubles of one record
    size_t shmem() const { return block() * sizeof(unsigned long long); }             // the LDS counters of a workgroup
    void check(const sphx_params &prm, const sphx_profile_series_config *cfg, int M);
    void alloc(const ProfileSeries &checked, int M);
    void zero(hipStream_t st) { isum.zero(st); head.zero(st); }  // (the counters: records beyond n_records are never read)
    void release() { isum.release(); times.release(); records.release(); head.release(); }
    void read(hipStream_t st, int capacity, double *times, double *records, int *n_records, int64_t *n_dropped, bool drain);
};

// Pair-distance statistics (sphx_ctx_pair_dist_*, sphx_batch_pair_dist_*; sphx_pair_dist.hpp) of a context or of the M members
// of a batch: one configuration, member m's integer sums at m * block() -- [n_bands][kinds][n_bins] counts, [n_bands] centres,
// [n_bands] r2_min bit patterns -- and its head at m.
struct PairDist {
    bool on = false;
    int members = 1;
    sphx_pair_dist_config cfg{};
    int n_bins = 0, n_bands = 1;  // (n_bands counts band 0)
    int kinds = 1;                // 2: a fluid-wall histogram beside the fluid-fluid one
    double r_max = 0.0;           // the range in force (cfg.r_max = 0: 2h)
    DevBuf<unsigned long long> sums;
    DevBuf<PairDistHead> head;
    std::vector<unsigned long long> empty;  // what zero() writes: zero counts, r2_min = +inf

    size_t counters() const { return (size_t)n_bands * (size_t)kinds * (size_t)n_bins; }
    size_t block() const { return counters() + 2 * (size_t)n_bands; }                  // the words of one member
    size_t shmem() const { return block() * sizeof(unsigned long long); }              // the LDS counters of a workgroup
    void check(const sphx_params &prm, const sphx_pair_dist_config *cfg, int M, bool has_walls);
    void alloc(const PairDist &checked, int M);
    void zero(hipStream_t st);
    void release() { sums.release(); head.release(); }
    void read(hipStream_t st, int band, int stride, int64_t *ff, int64_t *fw, int64_t *centres, double *r2_min, int64_t *n_samples,
              double *t_first, double *t_last) const;
};

// Gradient statistics (sphx_ctx_grad_stats_*, sphx_batch_grad_stats_*; sphx_grad_stats.hpp) of a context or of the M members of
// a batch: one configuration, bins and bands as FlowStats has them, member m's int64 sums of the sample in flight and its
// running sums at m * block() -- [n_bands][n_bins][kGradFields] -- and its head at m.
struct GradStats {
    bool on = false;
    int members = 1;
    sphx_grad_stats_config cfg{};
    int n_bins = 0, n_bands = 1;  // (n_bands counts band 0)
    bool walls = false;           // with_walls, and the channel holds wall particles
    DevBuf<unsigned long long> isum;
    DevBuf<double> dsum;
    DevBuf<GradStatsHead> head;

    size_t row() const { return (size_t)n_bins * kGradFields; }   // the sums of one band ...
    size_t block() const { return (size_t)n_bands * row(); }      // ... and of one member
    size_t shmem() const { return block() * sizeof(unsigned long long); }  // the LDS counters of a workgroup
    void check(const sphx_params &prm, const sphx_grad_stats_config *cfg, bool has_walls);
    void alloc(const GradStats &checked, int M);
    void zero(hipStream_t st) { isum.zero(st); dsum.zero(st); head.zero(st); }
    void release() { isum.release(); dsum.release(); head.release(); }
    void read(hipStream_t st, int band, int stride, double *sums, int64_t *n_samples, double *t_first, double *t_last) const;
};

// Particle tracers (sphx_ctx_tracers_*, sphx_batch_tracers_*; sphx_tracers.hpp) of a context or of the M members of a batch: one
// configuration and one id list, member m's times at m * cfg.capacity * 2, its values at m * cfg.capacity * row(), its head at
// m; the table index_of [n_fluid] is shared.  Of a slab of a ring (sphx_slab_tracers_*): cfg and ids are the ring's list, the
// same on every rank; the rows are dense -- T columns, NaN (byte 0xFF, nan_fill) where the slab was not the owner at that
// step -- and n_owned [capacity] holds the tracers the slab met per record.
struct Tracers {
    bool on = false;
    int members = 1;
    sphx_tracers_config cfg{};    // (cfg.ids: nullptr -- the ids are copied)
    std::vector<int32_t> ids;     // [n_tracers] as the caller gave them
    int n_fluid = 0;
    bool part = false;            // a slab's: a column is written only while the slab owns the particle
    DevBuf<int> index_of;
    DevBuf<double> times, values;
    DevBuf<long long> n_owned;    // (a slab's only)
    DevBuf<TracerHead> head;

    size_t row() const { return (size_t)cfg.n_tracers * kTracerFields; }  // the values of one record
    void check(int n_fluid, int n_total, const sphx_tracers_config *cfg, int M);
    void alloc(const Tracers &checked, int M, hipStream_t st);
    void zero(hipStream_t st) { head.zero(st); }  // (the counters: records beyond n_records are never read)
    void release() { index_of.release(); times.release(); values.release(); n_owned.release(); head.release(); }
    void nan_fill(hipStream_t st, size_t rows);  // a slab's: the first `rows` rows of values read NaN again
    void read(hipStream_t st, int capacity, double *times, double *values, int *n_records, int64_t *n_dropped, int64_t *n_missing,
              bool drain, int64_t *n_owned = nullptr);
};

// Density statistics (sphx_ctx_dens_stats_*, sphx_batch_dens_stats_*; sphx_dens_stats.hpp) of a context or of the M members of
// a batch: one configuration, bins and bands as FlowStats has them, member m's int64 sums of the sample in flight and its
// running sums at m * block() -- [n_bands][n_bins][kDensFields], then [n_bands][n_hist + 2] -- its running keys of d_max and
// -d_min at m * kblock() -- [n_bands][n_bins][kDensKeys], 0: no particle yet -- and its head at m.
struct DensStats {
    bool on = false;
    int members = 1;
    sphx_dens_stats_config cfg{};
    int n_bins = 0, n_bands = 1;  // (n_bands counts band 0)
    int e = -1;                   // 2^e >= cfg.delta_bound
    DevBuf<unsigned long long> isum, keys;
    DevBuf<double> dsum;
    DevBuf<DensStatsHead> head;

    size_t row() const { return (size_t)n_bins * kDensFields; }              // the binned sums of one band
    size_t hrow() const { return (size_t)cfg.n_hist + 2; }                   // the histogram of one band, below and above
    size_t block() const { return dens_sum_words(n_bands, n_bins, cfg.n_hist); }  // the sums of one member ...
    size_t kblock() const { return dens_key_words(n_bands, n_bins); }        // ... and its keys
    size_t shmem() const { return (block() + kblock()) * sizeof(unsigned long long); }  // the LDS of a workgroup
    void check(const sphx_params &prm, const sphx_dens_stats_config *cfg);
    void alloc(const DensStats &checked, int M);
    void zero(hipStream_t st) { isum.zero(st); keys.zero(st); dsum.zero(st); head.zero(st); }
    void release() { isum.release(); keys.release(); dsum.release(); head.release(); }
    void read(hipStream_t st, int m, int band, int stride, double *sums, int64_t *hist, int64_t *below, int64_t *above, int64_t *n_samples,
              double *t_first, double *t_last) const;
};

// Mode amplitudes (sphx_ctx_modes_*, sphx_batch_modes_*; sphx_modes.hpp) of a context or of the M members of a batch: one
// configuration, member m's int64 sums of the sample in flight at m * block(), its times at m * cfg.capacity * 2, its records
// at m * cfg.capacity * block(), its head at m.
struct Modes {
    bool on = false;
    int members = 1;
    sphx_modes_config cfg{};
    DevBuf<unsigned long long> isum;
    DevBuf<double> times, records;
    DevBuf<ModesHead> head;

    size_t block() const { return (size_t)(cfg.mx + 1) * (size_t)(cfg.ny + 1) * kModeSums; }  // the doubles of one record
    size_t shmem() const { return block() * sizeof(unsigned long long); }                     // the LDS counters of a workgroup
    int groups() const { return (cfg.mx + 1) * modes_runs(cfg.ny); }                          // what a workgroup serves one of
    void check(const sphx_modes_config *cfg, int M);
    void alloc(const Modes &checked, int M);
    void zero(hipStream_t st) { isum.zero(st); head.zero(st); }  // (the counters: records beyond n_records are never read)
    void release() { isum.release(); times.release(); records.release(); head.release(); }
    void read(hipStream_t st, int capacity, double *times, double *records, int *n_records, int64_t *n_dropped, bool drain);
};

// the samplers that are on, behind step slot q, which ran on layout l: statistics, history, field map, probes, profile series,
// pair statistics, gradient statistics, tracers, density statistics, mode amplitudes (sphx_samplers.hpp)
void launch_slot_samplers(sphx_ctx *c, int q, int l, bool rebuild);

}  // namespace sphx
