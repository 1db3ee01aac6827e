// sphx_sampler_state.hpp -- host state of the ten slot samplers ("Slot samplers"), part of the
// sphx_resident.hip translation unit: what sphx_ctx holds of each -- flow statistics (kernels: sphx_flow_stats.hpp), step history
// (sphx_history.hpp), field map (sphx_field_map.hpp), point probes (sphx_probes.hpp), profile series (sphx_profile_series.hpp),
// pair statistics (sphx_pair_dist.hpp), gradient statistics (sphx_grad_stats.hpp), particle tracers (sphx_tracers.hpp), density
// statistics (sphx_dens_stats.hpp) and mode amplitudes (sphx_modes.hpp).  Every sampler is two structs: its SHAPE -- the
// checked configuration and what check() derives from it, host values only, what the kernel arguments and the read-outs are
// computed from -- and, derived from it, the sampler itself: on / members, the device buffers that alloc() sizes from the
// shape, and the sampler's identifiers and message texts (names).  check() fills a shape or throws SPHX:<stem>:config and
// touches nothing else; alloc(checked, M, st) takes the checked shape over WHOLE, in one assignment, so a value check() derives
// cannot be forgotten on the way to the kernel.  Launches, lifecycle and entry points: sphx_samplers.hpp.
#pragma once
#include <functional>

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

// identifier stem (SPHX:<stem>:slab / :disabled / :config / :state / :range / :capacity) and message texts of a sampler
struct SamplerNames {
    const char *stem;
    const char *no_slab;    // a context's entry point on a slab context
    const char *off;        // ... "context", "batch" or "slab"
    const char *no_memory;  // enable, out of device memory: SPHX_ERR_ARG / SPHX:<stem>:config with this text in front of the
                            // allocator's; nullptr: the allocator's error goes out as it is
};

// Flow statistics (sphx_ctx_flow_stats_*, sphx_batch_flow_stats_*, sphx_slab_flow_stats_*) of a context or of the M members of
// a batch: one configuration, running sums and heads in M blocks (member m's sums at m * block(), its head at m).
struct FlowStatsShape {
    sphx_flow_stats_config cfg{};
    int n_bins = 0, n_bands = 1;  // (n_bands counts band 0)

    size_t row() const { return (size_t)n_bins * kStatsFields; }  // the sums of one band ...
    size_t block() const { return (size_t)n_bands * row(); }      // ... and of one member
    size_t shmem() const { return block() * sizeof(unsigned long long); }  // the LDS counters of a workgroup
    void check(const sphx_params &prm, const sphx_flow_stats_config *cfg);
};
struct FlowStats : FlowStatsShape {
    static constexpr SamplerNames names{"Stats", "flow statistics are not available on slab contexts",
                                        "flow statistics are not enabled on this ", nullptr};
    bool on = false;
    int members = 1;
    DevBuf<unsigned long long> isum;
    DevBuf<double> dsum;
    DevBuf<FlowStatsHead> head;

    void alloc(const FlowStatsShape &checked, int M, hipStream_t st);
    void zero(hipStream_t st) { isum.zero(st); dsum.zero(st); head.zero(st); }
    void release() { isum.release(); dsum.release(); head.release(); }
    void read(hipStream_t st, int band, int stride, bool sums, double *const out[kStatsFields], int64_t *n_samples, double *t_first,
              double *t_last) const;
};

// Step history (sphx_ctx_history_*, sphx_batch_history_*, sphx_slab_history_*) of a context or of the M members of a batch: one
// configuration, member m's records at m * cfg.capacity * kHistoryFields, its partials at m * kHistoryMaxBlocks *
// kHistorySums, its head at m.
struct HistoryShape {
    sphx_history_config cfg{};

    void check(const sphx_history_config *cfg, int M);
};
struct History : HistoryShape {
    static constexpr SamplerNames names{"History", "the step history is not available on slab contexts",
                                        "the step history is not enabled on this ", "the record buffer could not be set up: "};
    bool on = false;
    int members = 1;
    DevBuf<double> records, part;
    DevBuf<HistoryHead> head;

    void alloc(const HistoryShape &checked, int M, hipStream_t st);
    void zero(hipStream_t st) { head.zero(st); }  // (the counters: records beyond n_records are never read)
    void release() { records.release(); part.release(); head.release(); }
    void read(hipStream_t st, int capacity, double *records, int *n_records, int64_t *n_dropped, bool drain);
};

// Velocity-field map (sphx_ctx_field_map_*, sphx_batch_field_map_*) of a context or of the M members of a batch: one
// configuration and shape, member m's six planes at m * block(), its head at m.  Of a slab of a ring
// (sphx_slab_field_map_*): nx x ny is the ring's grid, the planes hold the block of node columns i_lo <= i < i_hi the slab owns.
struct FieldMapShape {
    sphx_field_map_config cfg{};
    int nx = 0, ny = 0;  // the shape in force (cfg.nx / cfg.ny = 0: the reference's)
    bool part = false;   // a slab's: the planes are those of the columns [i_lo, i_hi) only (possibly none)
    int i_lo = 0, i_hi = 0;

    int cols() const { return part ? i_hi - i_lo : nx;  }  // node columns held
    size_t nodes() const { return (size_t)cols() * (size_t)ny; }
    size_t block() const { return nodes() * kFieldPlanes; }  // the planes of one member
    void check(const sphx_params &prm, const sphx_field_map_config *cfg, int M);
};
struct FieldMap : FieldMapShape {
    static constexpr SamplerNames names{"Field", "field maps are not available on slab contexts", "the field map is not enabled on this ",
                                        "the map could not be set up: "};
    bool on = false;
    int members = 1;
    DevBuf<double> planes;
    DevBuf<FieldMapHead> head;

    void alloc(const FieldMapShape &checked, int M, hipStream_t st);
    void zero(hipStream_t st) { planes.zero(st); head.zero(st); }
    void release() { planes.release(); head.release(); }
    void read(hipStream_t st, int stride, double *const out[kFieldPlanes], int64_t *n_samples, double *t_first, double *t_last) const;
};

// Point probes (sphx_ctx_probes_*, sphx_batch_probes_*) of a context or of the M members of a batch: one configuration and one
// set of points, member m's times at m * cfg.capacity * 2, its values at m * cfg.capacity * row(), its head at m.  Of a slab
// of a ring (sphx_slab_probes_*): cfg and folded are the ring's list, the same on every rank; the device holds the probes the
// slab owns -- those of `index`, in the ring's order -- and their values.
struct ProbesShape {
    sphx_probes_config cfg{};     // (cfg.points: nullptr -- the points are copied)
    std::vector<double> folded;   // [n_points][2]: x folded into [0, DL), y
    bool part = false;            // a slab's: points / values are those of the probes of `index` only (possibly none)
    std::vector<int> index;       // [n_owned] positions of the owned probes in the ring's list, ascending

    int held() const { return part ? (int)index.size() : cfg.n_points; }  // probes on the device
    size_t row() const { return (size_t)held() * kProbeFields; }          // the values of one record
    void check(const sphx_params &prm, const sphx_probes_config *cfg, int M);
};
struct Probes : ProbesShape {
    static constexpr SamplerNames names{"Probe", "point probes are not available on slab contexts",
                                        "point probes are not enabled on this ", "the record buffer could not be set up: "};
    bool on = false;
    int members = 1;
    DevBuf<double2> points;
    DevBuf<double> times, values;
    DevBuf<ProbeHead> head;

    void alloc(const ProbesShape &checked, int M, hipStream_t st);
    void zero(hipStream_t st) { head.zero(st); }  // (the counters: records beyond n_records are never read)
    void release() { points.release(); times.release(); values.release(); head.release(); }
    void read(hipStream_t st, int capacity, double *times, double *values, int *n_records, int64_t *n_dropped, bool drain);
};

// Profile series (sphx_ctx_profile_series_*, sphx_batch_profile_series_*, sphx_slab_pseries_*) of a context or of the M
// members of a batch: one configuration, bins and bands as FlowStats has them, member m's int64 sums of the sample in flight
// at m * block(), its times at m * cfg.capacity * 2, its records at m * cfg.capacity * block(), its head at m.
struct ProfileSeriesShape {
    sphx_profile_series_config cfg{};
    int n_bins = 0, n_bands = 1;  // (n_bands counts band 0)

    size_t block() const { return (size_t)n_bands * (size_t)n_bins * kStatsFields; }  // the doubles of one record
    size_t shmem() const { return block() * sizeof(unsigned long long); }             // the LDS counters of a workgroup
    void check(const sphx_params &prm, const sphx_profile_series_config *cfg, int M);
};
struct ProfileSeries : ProfileSeriesShape {
    static constexpr SamplerNames names{"ProfileSeries", "the profile series of a slab is sphx_slab_pseries_* (include/sphx.h section 3a)",
                                        "the profile series is not enabled on this ", "the record buffer could not be set up: "};
    bool on = false;
    int members = 1;
    DevBuf<unsigned long long> isum;
    DevBuf<double> times, records;
    DevBuf<ProfileSeriesHead> head;

    void alloc(const ProfileSeriesShape &checked, int M, hipStream_t st);
    void zero(hipStream_t st) { isum.zero(st); head.zero(st); }  // (the counters: records beyond n_records are never read)
    void release() { isum.release(); times.release(); records.release(); head.release(); }
    void read(hipStream_t st, int capacity, double *times, double *records, int *n_records, int64_t *n_dropped, bool drain);
};

// Pair-distance statistics (sphx_ctx_pair_dist_*, sphx_batch_pair_dist_*, sphx_slab_pairs_*) of a context or of the M members
// of a batch: one configuration, member m's integer sums at m * block() -- [n_bands][kinds][n_bins] counts, [n_bands] centres,
// [n_bands] r2_min bit patterns -- and its head at m.
struct PairDistShape {
    sphx_pair_dist_config cfg{};
    int n_bins = 0, n_bands = 1;  // (n_bands counts band 0)
    int kinds = 1;                // 2: a fluid-wall histogram beside the fluid-fluid one
    double r_max = 0.0;           // the range in force (cfg.r_max = 0: 2h)

    size_t counters() const { return (size_t)n_bands * (size_t)kinds * (size_t)n_bins; }
    size_t block() const { return counters() + 2 * (size_t)n_bands; }                  // the words of one member
    size_t shmem() const { return block() * sizeof(unsigned long long); }              // the LDS counters of a workgroup
    void check(const sphx_params &prm, const sphx_pair_dist_config *cfg, bool has_walls);
};
struct PairDist : PairDistShape {
    static constexpr SamplerNames names{"PairDist", "the pair statistics of a slab are sphx_slab_pairs_* (include/sphx.h section 3a)",
                                        "pair statistics are not enabled on this ", "the sums could not be set up: "};
    bool on = false;
    int members = 1;
    DevBuf<unsigned long long> sums;
    DevBuf<PairDistHead> head;
    std::vector<unsigned long long> empty;  // what zero() writes: zero counts, r2_min = +inf

    void alloc(const PairDistShape &checked, int M, hipStream_t st);
    void zero(hipStream_t st);
    void release() { sums.release(); head.release(); }
    void read(hipStream_t st, int band, int stride, int64_t *ff, int64_t *fw, int64_t *centres, double *r2_min, int64_t *n_samples,
              double *t_first, double *t_last) const;
};

// Gradient statistics (sphx_ctx_grad_stats_*, sphx_batch_grad_stats_*, sphx_slab_gstats_*) of a context or of the M members of
// a batch: one configuration, bins and bands as FlowStats has them, member m's int64 sums of the sample in flight and its
// running sums at m * block() -- [n_bands][n_bins][kGradFields] -- and its head at m.
struct GradStatsShape {
    sphx_grad_stats_config cfg{};
    int n_bins = 0, n_bands = 1;  // (n_bands counts band 0)
    bool walls = false;           // with_walls, and the channel holds wall particles

    size_t row() const { return (size_t)n_bins * kGradFields; }   // the sums of one band ...
    size_t block() const { return (size_t)n_bands * row(); }      // ... and of one member
    size_t shmem() const { return block() * sizeof(unsigned long long); }  // the LDS counters of a workgroup
    void check(const sphx_params &prm, const sphx_grad_stats_config *cfg, bool has_walls);
};
struct GradStats : GradStatsShape {
    static constexpr SamplerNames names{"GradStats", "the gradient statistics of a slab are sphx_slab_gstats_* (include/sphx.h section 3a)",
                                        "gradient statistics are not enabled on this ", "the sums could not be set up: "};
    bool on = false;
    int members = 1;
    DevBuf<unsigned long long> isum;
    DevBuf<double> dsum;
    DevBuf<GradStatsHead> head;

    void alloc(const GradStatsShape &checked, int M, hipStream_t st);
    void zero(hipStream_t st) { isum.zero(st); dsum.zero(st); head.zero(st); }
    void release() { isum.release(); dsum.release(); head.release(); }
    void read(hipStream_t st, int band, int stride, double *sums, int64_t *n_samples, double *t_first, double *t_last) const;
};

// Particle tracers (sphx_ctx_tracers_*, sphx_batch_tracers_*) of a context or of the M members of a batch: one configuration
// and one id list, member m's times at m * cfg.capacity * 2, its values at m * cfg.capacity * row(), its head at m; the table
// index_of [n_fluid] is shared.  Of a slab of a ring (sphx_slab_tracers_*): cfg and ids are the ring's list, the same on every
// rank; the rows are dense -- T columns, NaN (byte 0xFF, nan_fill) where the slab was not the owner at that step -- and
// n_owned [capacity] holds the tracers the slab met per record.
struct TracersShape {
    sphx_tracers_config cfg{};    // (cfg.ids: nullptr -- the ids are copied)
    std::vector<int32_t> ids;     // [n_tracers] as the caller gave them
    int n_fluid = 0;
    bool part = false;            // a slab's: a column is written only while the slab owns the particle

    size_t row() const { return (size_t)cfg.n_tracers * kTracerFields; }  // the values of one record
    void check(int n_fluid, int n_total, const sphx_tracers_config *cfg, int M);
};
struct Tracers : TracersShape {
    static constexpr SamplerNames names{"Tracers", "the tracers of a slab are sphx_slab_tracers_* (include/sphx.h section 3a)",
                                        "particle tracers are not enabled on this ", "the record buffer could not be set up: "};
    bool on = false;
    int members = 1;
    DevBuf<int> index_of;
    DevBuf<double> times, values;
    DevBuf<long long> n_owned;    // (a slab's only)
    DevBuf<TracerHead> head;

    void alloc(const TracersShape &checked, int M, hipStream_t st);
    void zero(hipStream_t st) { head.zero(st); }  // (the counters: records beyond n_records are never read)
    void release() { index_of.release(); times.release(); values.release(); n_owned.release(); head.release(); }
    void nan_fill(hipStream_t st, size_t rows);  // a slab's: the first `rows` rows of values read NaN again
    void read(hipStream_t st, int capacity, double *times, double *values, int *n_records, int64_t *n_dropped, int64_t *n_missing,
              bool drain, int64_t *n_owned = nullptr);
};

// Density statistics (sphx_ctx_dens_stats_*, sphx_batch_dens_stats_*, sphx_slab_dstats_*) of a context or of the M members of
// a batch: one configuration, bins and bands as FlowStats has them, member m's int64 sums of the sample in flight and its
// running sums at m * block() -- [n_bands][n_bins][kDensFields], then [n_bands][n_hist + 2] -- its running keys of d_max and
// -d_min at m * kblock() -- [n_bands][n_bins][kDensKeys], 0: no particle yet -- and its head at m.
struct DensStatsShape {
    sphx_dens_stats_config cfg{};
    int n_bins = 0, n_bands = 1;  // (n_bands counts band 0)
    int e = -1;                   // 2^e >= cfg.delta_bound

    size_t row() const { return (size_t)n_bins * kDensFields; }              // the binned sums of one band
    size_t hrow() const { return (size_t)cfg.n_hist + 2; }                   // the histogram of one band, below and above
    size_t block() const { return dens_sum_words(n_bands, n_bins, cfg.n_hist); }  // the sums of one member ...
    size_t kblock() const { return dens_key_words(n_bands, n_bins); }        // ... and its keys
    size_t shmem() const { return (block() + kblock()) * sizeof(unsigned long long); }  // the LDS of a workgroup
    void check(const sphx_params &prm, const sphx_dens_stats_config *cfg);
};
struct DensStats : DensStatsShape {
    static constexpr SamplerNames names{"DensStats", "the density statistics of a slab are sphx_slab_dstats_* (include/sphx.h section 3a)",
                                        "density statistics are not enabled on this ", "the sums could not be set up: "};
    bool on = false;
    int members = 1;
    DevBuf<unsigned long long> isum, keys;
    DevBuf<double> dsum;
    DevBuf<DensStatsHead> head;

    void alloc(const DensStatsShape &checked, int M, hipStream_t st);
    void zero(hipStream_t st) { isum.zero(st); keys.zero(st); dsum.zero(st); head.zero(st); }
    void release() { isum.release(); keys.release(); dsum.release(); head.release(); }
    void read(hipStream_t st, int m, int band, int stride, double *sums, int64_t *hist, int64_t *below, int64_t *above, int64_t *n_samples,
              double *t_first, double *t_last) const;
};

// Mode amplitudes (sphx_ctx_modes_*, sphx_batch_modes_*) of a context or of the M members of a batch: one configuration,
// member m's int64 sums of the sample in flight at m * block(), its times at m * cfg.capacity * 2, its records at
// m * cfg.capacity * block(), its head at m.
struct ModesShape {
    sphx_modes_config cfg{};

    size_t block() const { return (size_t)(cfg.mx + 1) * (size_t)(cfg.ny + 1) * kModeSums; }  // the doubles of one record
    size_t shmem() const { return block() * sizeof(unsigned long long); }                     // the LDS counters of a workgroup
    int groups() const { return (cfg.mx + 1) * modes_runs(cfg.ny); }                          // what a workgroup serves one of
    void check(const sphx_modes_config *cfg, int M);
};
struct Modes : ModesShape {
    static constexpr SamplerNames names{"Modes", "mode amplitudes are not available on slab contexts",
                                        "mode amplitudes are not enabled on this ", "the record buffer could not be set up: "};
    bool on = false;
    int members = 1;
    DevBuf<unsigned long long> isum;
    DevBuf<double> times, records;
    DevBuf<ModesHead> head;

    void alloc(const ModesShape &checked, int M, hipStream_t st);
    void zero(hipStream_t st) { isum.zero(st); head.zero(st); }  // (the counters: records beyond n_records are never read)
    void release() { isum.release(); times.release(); records.release(); head.release(); }
    void read(hipStream_t st, int capacity, double *times, double *records, int *n_records, int64_t *n_dropped, bool drain);
};

// the samplers that are on, behind step slot q, which ran on layout l: statistics, history, field map, probes, profile series,
// pair statistics, gradient statistics, tracers, density statistics, mode amplitudes (sphx_samplers.hpp)
void launch_slot_samplers(sphx_ctx *c, int q, int l, bool rebuild);

}  // namespace sphx
